"""SarHeadEngine: the SAR hand-mesh head of the RootNet checkpoint (SAIGB + GBBMR + SoftHeatmap, rootnet/Model_RGB.py:76-222)
on libhamer_hip, for all hands of a call at once, plus the post-processing of EstimateRGB.run (:428-480) in one launch.

Load-time work: the ``head.*`` keys are mapped, the four Laplacians L = A / (rowsum(A) + 1e-5) are formed in fp32 as torch
does, and the weights are padded (K to a multiple of 32 with zeros) and cast to f16.  Activations stay node-major across the
batch ([778][B][C]); see csrc/sar.hip.  precise=True is the fp32 route (csrc/sar_f32.hip): fp32 weights, an fp32 workspace
and the ``_f32`` entry points, deterministic and batch-invariant."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .. import lib as L

NV, NJ, NT, CELLS = 778, 21, 799, 1024
KG = 544            # SAIGB row: 512 features + 3 template + 29 zeros
LDL = 800           # Laplacian row stride: 778 + 22 zero columns


def laplacian(adj: torch.Tensor) -> torch.Tensor:
    """GraphConv.laplacian (:104-108) in fp32: 1 / (rowsum(A) + 1e-5) * A."""
    a = adj.float()
    d = torch.sum(a, 1, keepdim=True) + 1e-5
    return 1 / d * a


def head_keys():
    """Every ``head.*`` key the engine reads (the resnet34 SAR head's full state dict)."""
    keys = ["head.saigb.template", "head.saigb.group.0.weight", "head.saigb.group.0.bias"]
    for br in ("reg_xy", "reg_z"):
        for layer in ("0", "3"):
            keys += [f"head.gbbmr.{br}.{layer}.{n}" for n in ("fc.weight", "fc.bias", "adj")]
    for m in ("mesh2pose_hm", "mesh2pose_dm"):
        keys += [f"head.gbbmr.{m}.weight", f"head.gbbmr.{m}.bias"]
    keys += ["head.gbbmr.soft_heatmap." + n for n in ("beta.weight", "wx", "wy")]
    return keys


def _pad(w: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    out = torch.zeros(rows, cols, dtype=torch.float32)
    out[:w.shape[0], :w.shape[1]] = w.float()
    return out


def host_weights(sd: Dict[str, torch.Tensor], in_channels: int = 512) -> Dict[str, torch.Tensor]:
    """The engine's operands on the host, fp32 (cast to f16 / kept fp32 on upload): named by what the kernels take.
    in_channels: the backbone's feature channels (512: ResNet-34, 1024: ConvNeXt-base), the K of SAIGB's 1 x 1 convolution."""
    missing = [k for k in head_keys() if k not in sd]
    if missing:
        raise KeyError(f"SAR head weights missing from the checkpoint: {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    h = "head."
    if tuple(sd[h + "saigb.group.0.weight"].shape[:2]) != (8 * NV, in_channels):
        raise ValueError(f"head.saigb.group.0.weight has shape {tuple(sd[h + 'saigb.group.0.weight'].shape)}; a backbone of "
                         f"{in_channels} channels needs ({8 * NV}, {in_channels}, 1, 1)")
    w = {"saigb_w": sd[h + "saigb.group.0.weight"].float().reshape(8 * NV, in_channels),
         "saigb_b": sd[h + "saigb.group.0.bias"].float(),
         "template": sd[h + "saigb.template"].float().reshape(NV, 3)}
    for br in ("xy", "z"):
        pre = f"{h}gbbmr.reg_{br}."
        w[f"{br}.lap0"] = _pad(laplacian(sd[pre + "0.adj"]), NV, LDL)
        w[f"{br}.w0"] = _pad(sd[pre + "0.fc.weight"], CELLS, KG)
        w[f"{br}.b0"] = sd[pre + "0.fc.bias"].float()
        w[f"{br}.lap1"] = _pad(laplacian(sd[pre + "3.adj"]), NV, LDL)
        w[f"{br}.w1"] = sd[pre + "3.fc.weight"].float()
        w[f"{br}.b1"] = sd[pre + "3.fc.bias"].float()
    for br, m in (("xy", "mesh2pose_hm"), ("z", "mesh2pose_dm")):
        w[f"{br}.m2p_w"] = sd[f"{h}gbbmr.{m}.weight"].float().reshape(NJ, NV)
        w[f"{br}.m2p_b"] = sd[f"{h}gbbmr.{m}.bias"].float().reshape(NJ)
    w["beta"] = sd[h + "gbbmr.soft_heatmap.beta.weight"].float().reshape(NT)
    w["wx"] = sd[h + "gbbmr.soft_heatmap.wx"].float().reshape(CELLS)
    w["wy"] = sd[h + "gbbmr.soft_heatmap.wy"].float().reshape(CELLS)
    return w


_F16_KEYS = ("saigb_w", "xy.lap0", "xy.w0", "xy.lap1", "xy.w1", "z.lap0", "z.w0", "z.lap1", "z.w1")


class SarHeadEngine:
    def __init__(self, net_sd: Dict[str, torch.Tensor], device="cuda", precise: bool = False, in_channels: int = 512):
        if in_channels not in (512, 1024):
            raise ValueError(f"SarHeadEngine: in_channels {in_channels} (512: ResNet-34 features, 1024: ConvNeXt-base features)")
        if precise and in_channels != 512:
            raise ValueError("SarHeadEngine: the fp32 route of the 1024-channel (ConvNeXt) head does not exist yet")
        if not torch.cuda.is_available():
            raise L.HipLibraryError("SarHeadEngine needs an MI355X (HIP device); there is no CPU fallback")
        self.lib = L.load()
        self.device = torch.device(device)
        self.precise = bool(precise)
        self.in_channels = int(in_channels)
        self.act_dtype = torch.float32 if self.precise else torch.float16          # features, g, mix and h
        self.w = {k: v.to(self.device, torch.float16 if k in _F16_KEYS and not self.precise else torch.float32).contiguous()
                  for k, v in host_weights(net_sd, self.in_channels).items()}
        self._ws: Dict[int, Dict[str, torch.Tensor]] = {}
        f = "_f32" if self.precise else ""
        self._saigb, self._mix, self._linear = (getattr(self.lib, n + f) for n in ("hm_sar_saigb", "hm_sar_graph_mix", "hm_sar_linear"))

    def _workspace(self, B: int) -> Dict[str, torch.Tensor]:
        ws = self._ws.get(B)
        if ws is None:
            e = dict(device=self.device)
            ad = self.act_dtype
            ws = {"g": torch.empty(NV, B, KG, dtype=ad, **e),
                  "mix": torch.empty(NV, B * CELLS, dtype=ad, **e),                  # L . x of both layers (B * 544 fits too)
                  "h": torch.empty(NV * B, CELLS, dtype=ad, **e),
                  "xy": torch.empty(NT, B, CELLS, dtype=torch.float32, **e),
                  "z": torch.empty(NT, B, CELLS, dtype=torch.float32, **e)}
            self._ws = {B: ws}                                                       # keep one batch size's buffers
        return ws

    def saigb(self, feat: torch.Tensor) -> torch.Tensor:
        """feat (B, 8, 8, in_channels) NHWC, f16 (fp32 when precise) -> the init graph [778][B][544] in the same dtype (a view
        of the workspace)."""
        B = feat.shape[0]
        assert feat.shape[1:] == (8, 8, self.in_channels) and feat.dtype == self.act_dtype and feat.is_contiguous()
        g = self._workspace(B)["g"]
        if self.in_channels != 512:
            L.check(self.lib.hm_sar_saigb_ch(L.ptr(feat), L.ptr(self.w["saigb_w"]), L.ptr(self.w["saigb_b"]), L.ptr(self.w["template"]),
                                             L.ptr(g), B, self.in_channels, L.current_stream()), "hm_sar_saigb_ch")
            return g
        L.check(self._saigb(L.ptr(feat), L.ptr(self.w["saigb_w"]), L.ptr(self.w["saigb_b"]), L.ptr(self.w["template"]),
                            L.ptr(g), B, L.current_stream()), "hm_sar_saigb")
        return g

    def branch(self, g: torch.Tensor, br: str, out: torch.Tensor) -> torch.Tensor:
        """reg_xy / reg_z (:146-157) -> out[0:778] = second-layer logits, [778][B][1024] f32."""
        B = g.shape[1]
        ws, w, s = self._workspace(B), self.w, L.current_stream()
        mix, h = ws["mix"], ws["h"]
        L.check(self._mix(L.ptr(w[br + ".lap0"]), LDL, L.ptr(g), B * KG, L.ptr(mix), s), "hm_sar_graph_mix")
        L.check(self._linear(L.ptr(mix), NV * B, KG, L.ptr(w[br + ".w0"]), L.ptr(w[br + ".b0"]), L.ptr(h), CELLS, 0, s), "hm_sar_linear")
        L.check(self._mix(L.ptr(w[br + ".lap1"]), LDL, L.ptr(h), B * CELLS, L.ptr(mix), s), "hm_sar_graph_mix")
        L.check(self._linear(L.ptr(mix), NV * B, CELLS, L.ptr(w[br + ".w1"]), L.ptr(w[br + ".b1"]), L.ptr(out), CELLS, 1, s),
                "hm_sar_linear")
        return out

    def soft_argmax(self, B: int, coords: Optional[torch.Tensor] = None) -> torch.Tensor:
        ws, w = self._workspace(B), self.w
        if coords is None:
            coords = torch.empty(B, NT, 3, device=self.device, dtype=torch.float32)
        L.check(self.lib.hm_sar_softargmax(L.ptr(ws["xy"]), L.ptr(ws["z"]), L.ptr(w["xy.m2p_w"]), L.ptr(w["xy.m2p_b"]),
                                           L.ptr(w["z.m2p_w"]), L.ptr(w["z.m2p_b"]), L.ptr(w["beta"]), L.ptr(w["wx"]), L.ptr(w["wy"]),
                                           L.ptr(coords), B, L.current_stream()), "hm_sar_softargmax")
        return coords

    def forward(self, feat: torch.Tensor) -> torch.Tensor:
        """SARhead.forward (:213-222): feat (B, 8, 8, 512) NHWC (RootNetEngine.features; f16, fp32 when precise) -> coords
        (B, 799, 3) f32:
        normalised xy, relative z; rows 778 .. 798 are the joints."""
        B = feat.shape[0]
        g = self.saigb(feat)
        ws = self._workspace(B)
        self.branch(g, "xy", ws["xy"])
        self.branch(g, "z", ws["z"])
        return self.soft_argmax(B)

    def postprocess(self, coords: torch.Tensor, hands, root: Optional[torch.Tensor] = None, depth: Optional[torch.Tensor] = None,
                    P: int = 256):
        """hm_sar_postprocess: coords (B, 799, 3), hands: a sequence of lib.SarHand -> (uvd, xyz), each (B, 799, 3) f32."""
        B = coords.shape[0]
        arr = (L.SarHand * B)(*hands)
        hd = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        uvd = torch.empty(B, NT, 3, device=self.device, dtype=torch.float32)
        xyz = torch.empty_like(uvd)
        if root is not None:
            root = root.to(self.device, torch.float32).contiguous()
        L.check(self.lib.hm_sar_postprocess(L.ptr(coords), L.ptr(hd), L.ptr(root), L.ptr(depth), L.ptr(uvd), L.ptr(xyz), B, P,
                                            L.current_stream()), "hm_sar_postprocess")
        return uvd, xyz


def sar_hand(bb2img: np.ndarray, K, img_w: int, img_h: int, flip: bool, depth_box: float = 0.3, depth_offset: int = -1,
             depth_wh=(0, 0)) -> L.SarHand:
    h = L.SarHand()
    for i, v in enumerate(np.asarray(bb2img, np.float32).reshape(6)):
        h.bb2img[i] = float(v)
    h.depth_box, h.flip, h.img_w, h.img_h = float(depth_box), int(bool(flip)), int(img_w), int(img_h)
    h.depth_w, h.depth_h, h.depth_offset = int(depth_wh[0]), int(depth_wh[1]), int(depth_offset)
    K = np.asarray(K, np.float64)
    h.fx, h.fy, h.fu, h.fv = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    return h
