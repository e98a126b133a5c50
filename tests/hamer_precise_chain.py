"""The truth the precise (fp32) HaMeR route is measured against: the oracle's own forward, evaluated in fp64 on the CPU.

``oracle.hamer_ref.hamer_forward`` is dtype-generic on its non-emulated path, so the chain is that very function called with
the state dict, the MANO parameters and the crops converted to double under ``torch.set_default_dtype(torch.float64)`` (its
constants -- the focal length vector, the decoder's zero token -- follow the default dtype).  Run with ``torch.float32`` it IS
the fp32 CPU oracle, bit for bit.  Test helper only: the package never imports it.
"""
from typing import Dict

import torch

from oracle import hamer_ref as R

# engine output name -> how to get it from the oracle's dictionary
ENGINE_KEYS = ("tokens", "pose6d", "betas", "pred_cam", "rotmats", "pred_vertices", "pred_keypoints_3d", "pred_cam_t",
               "pred_keypoints_2d")


def _cast(d: Dict, dtype) -> Dict:
    out = {}
    for k, v in d.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu()
            out[k] = v.to(dtype) if v.is_floating_point() else v
        else:
            out[k] = v
    return out


def chain_forward(sd: Dict, mp: Dict, img: torch.Tensor, cfg, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """hamer_forward in `dtype` on the CPU; every returned tensor has that dtype."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.no_grad():
            return R.hamer_forward(_cast(sd, dtype), _cast(mp, dtype), img.detach().cpu().to(dtype), cfg, emu=False)
    finally:
        torch.set_default_dtype(old)


def engine_view(o: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The oracle's dictionary under HamerEngine.forward's names and shapes (tokens as [B * 192][D])."""
    B = o["pose6d"].shape[0]
    return {
        "tokens": o["tokens"].reshape(B * o["tokens"].shape[1], -1),
        "pose6d": o["pose6d"], "betas": o["betas"], "pred_cam": o["pred_cam"],
        "rotmats": torch.cat([o["global_orient"], o["hand_pose"]], 1),
        "pred_vertices": o["pred_vertices"], "pred_keypoints_3d": o["pred_keypoints_3d"], "pred_cam_t": o["pred_cam_t"],
        "pred_keypoints_2d": o["pred_keypoints_2d"],
    }


def distances(got: Dict[str, torch.Tensor], truth: Dict[str, torch.Tensor], keys=ENGINE_KEYS) -> Dict[str, float]:
    """max |got - truth| per output, taken in fp64."""
    return {k: float((got[k].detach().cpu().double().reshape(truth[k].shape) - truth[k].double()).abs().max()) for k in keys}


def linear64(x: torch.Tensor, w: torch.Tensor, bias, epilogue: str, resid=None, resid_mod: int = 0):
    """fp64 value of hm_gemm_f32 and the per-output magnitude sum_k |x w| its error is measured against."""
    x64, w64 = x.double().cpu(), w.double().cpu()
    y = x64 @ w64.t()
    mag = x64.abs() @ w64.abs().t()
    if bias is not None:
        y = y + bias.double().cpu()
    if epilogue == "gelu":
        y = 0.5 * y * (1.0 + torch.erf(y * 0.5 ** 0.5))
    if epilogue == "resid":
        r = resid.double().cpu()
        y = y + (r[torch.arange(y.shape[0]) % resid_mod] if resid_mod else r)
    return y, mag
