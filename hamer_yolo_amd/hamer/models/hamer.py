"""HAMER model object with the call surface infer.py uses (reference: hamer/hamer/models/hamer.py:
``forward_step`` :99-156, ``forward`` :269-277).  All arithmetic is one hm_hamer_forward enqueue
(HamerEngine); this class assembles the reference's output dictionaries from the kernel outputs.
Training (losses, discriminator, Lightning hooks) is out of scope.
"""
from typing import Dict, Optional, Tuple

import torch

from ... import synth
from ...engine import HamerEngine
from ...lib import HipLibraryError
from .mano_wrapper import MANO


def engine_config(cfg, state_dict: Dict[str, torch.Tensor]) -> synth.HamerConfig:
    """The geometry HamerEngine needs, from ``model_config.yaml`` and the checkpoint's own tensor shapes -- and a clear
    error for every configuration of the reference that the HIP forward does not implement (rather than silently wrong
    outputs): the reference builds ``vit()`` = ViT-H/16 (backbones/vit.py:343-348), a transformer-decoder head fed the
    zero token (mano_head.py:31,:86), one IEF iteration (:81) and the 6-D rotation representation (:28-30)."""
    M = cfg.MODEL
    head = M.get("MANO_HEAD", {})
    if str(M.get("BACKBONE", {}).get("TYPE", "vit")) != "vit":
        raise ValueError(f"unsupported MODEL.BACKBONE.TYPE {M.BACKBONE.TYPE!r}: the HIP forward implements the ViT-H/16 backbone")
    if str(head.get("TYPE", "transformer_decoder")) != "transformer_decoder":
        raise ValueError(f"unsupported MODEL.MANO_HEAD.TYPE {head.get('TYPE')!r}")
    if str(head.get("JOINT_REP", "6d")) != "6d":
        raise ValueError("unsupported MODEL.MANO_HEAD.JOINT_REP: only the 6-D rotation representation is implemented")
    if str(head.get("TRANSFORMER_INPUT", "zero")) != "zero":
        raise ValueError("unsupported MODEL.MANO_HEAD.TRANSFORMER_INPUT: only the zero input token is implemented")
    if int(head.get("IEF_ITERS", 1)) != 1:
        raise ValueError("unsupported MODEL.MANO_HEAD.IEF_ITERS: one iteration is implemented (init_* folded into the read-out bias)")
    if int(cfg.MANO.get("NUM_HAND_JOINTS", 15)) != 15:
        raise ValueError("MANO.NUM_HAND_JOINTS must be 15")
    td = dict(head.get("TRANSFORMER_DECODER", {}))
    if str(td.get("norm", "layer")) != "layer":
        raise ValueError("unsupported TRANSFORMER_DECODER.norm: only LayerNorm is implemented")
    sd = state_dict
    pos = sd["backbone.pos_embed"]
    D = int(pos.shape[-1])
    depth = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("backbone.blocks."))
    pw = sd["backbone.patch_embed.proj.weight"]
    if D % 80 != 0 or tuple(pw.shape[1:]) != (3, 16, 16) or int(pos.shape[1]) != 193:
        raise ValueError(f"backbone geometry not supported: pos_embed {tuple(pos.shape)}, patch weight {tuple(pw.shape)} "
                         "(expected 192+1 tokens of a 256x192 window, 16x16 patches, head_dim 80)")
    mlp_ratio = int(sd["backbone.blocks.0.mlp.fc1.weight"].shape[0]) // D
    t = "mano_head.transformer."
    dim = int(sd[t + "pos_embedding"].shape[-1])
    ddepth = 1 + max(int(k[len(t):].split(".")[2]) for k in sd if k.startswith(t + "transformer.layers."))
    inner = int(sd[t + "transformer.layers.0.1.fn.to_q.weight"].shape[0])
    ctx = int(sd[t + "transformer.layers.0.1.fn.to_kv.weight"].shape[1])
    dec = synth.DecoderConfig(dim=dim, depth=ddepth, heads=int(td.get("heads", 8)), dim_head=int(td.get("dim_head", 64)),
                              mlp_dim=int(sd[t + "transformer.layers.0.2.fn.net.0.weight"].shape[0]), context_dim=ctx)
    if dec.inner != inner or ctx != D or int(td.get("depth", ddepth)) != ddepth or int(td.get("mlp_dim", dec.mlp_dim)) != dec.mlp_dim \
            or int(td.get("context_dim", ctx)) != ctx or int(td.get("dim", dim)) != dim:
        raise ValueError("model_config.yaml TRANSFORMER_DECODER does not match the checkpoint's decoder tensors "
                         f"(config {td}; checkpoint dim {dim}, depth {ddepth}, inner {inner}, mlp {dec.mlp_dim}, context {ctx})")
    if int(sd[t + "to_token_embedding.weight"].shape[1]) != 1 or int(sd["mano_head.decpose.weight"].shape[0]) != 96:
        raise ValueError("decoder input token / pose read-out shape not supported (zero token of width 1, 96 = 16 x 6-D rotations)")
    vit = synth.ViTConfig(embed_dim=D, depth=depth, heads=D // 80, mlp_ratio=mlp_ratio)
    return synth.HamerConfig(vit=vit, dec=dec, image_size=int(M.IMAGE_SIZE), focal_length=float(cfg.EXTRA.FOCAL_LENGTH))


class HAMER:
    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], mano: MANO, dtype=torch.float16,
                 hamer_cfg: Optional[synth.HamerConfig] = None, token_merge=False):
        # dtype=torch.float32 is the precise route: fp32 weights and activations on the fp32-input MFMA
        if dtype == torch.float32 and token_merge:
            raise ValueError("HAMER(dtype=torch.float32): token merging is not part of the precise fp32 route")
        self.cfg = cfg
        self.mano = mano
        self.dtype = dtype
        self.token_merge = token_merge
        self._sd = state_dict
        self._hc = hamer_cfg or engine_config(cfg, state_dict)
        self._engine: Optional[HamerEngine] = None
        self.check_fp16_range = True   # one calibration forward at .to(device) (2 ms); set False to skip
        self._ws = {}                  # HIP stream -> (capacity in hands, workspace): forwards on different streams may overlap
        self.device = torch.device("cpu")
        self.training = False

    # -- nn.Module-like surface used by hamer_inference.__init__ (infer.py:139-140)
    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise HipLibraryError("HAMER runs on an MI355X only: the HIP hot path has no CPU fallback")
        if self._engine is None or self.device != device:
            self._engine = HamerEngine(self._sd, self.mano.params, self._hc, device=device, dtype=self.dtype,
                                       token_merge=self.token_merge or None)
            # (the precise fp32 route has fp32's range: no check)
            # fp16 operands (the type that meets the 1e-3 bar) have a 65504 ceiling and no overflow detection: check once,
            # at load, that this checkpoint's activations fit; if not, take the wider exponent and say so
            if self.dtype == torch.float16 and self.check_fp16_range and not self._engine.calibration_is_finite():
                import warnings
                from ...engine import prescale_from_ranges
                # Round 4: keep the 11-bit operands.  A bf16 engine of the same checkpoint (fp32's exponent range) measures how
                # large every 16-bit activation class gets; powers of two folded into the weights bring each class back inside
                # fp16 (HamerEngine prescale: exact arithmetic, the same function).  bfloat16 operands -- 8 significant bits,
                # 1.2-1.9e-3 from the fp32 reference on theta / beta -- remain the last resort (and what token merging takes).
                self._engine = None
                probe = HamerEngine(self._sd, self.mano.params, self._hc, device=device, dtype=torch.bfloat16)
                if not probe.calibration_is_finite():
                    raise HipLibraryError("HAMER: non-finite outputs on the calibration crops with bfloat16 operands too: bad checkpoint?")
                eng = None
                if not self.token_merge:
                    try:
                        pre = prescale_from_ranges(probe.measure_ranges(), self._hc.vit.depth, self._hc.dec.depth)
                        eng = HamerEngine(self._sd, self.mano.params, self._hc, device=device, dtype=torch.float16, prescale=pre)
                        if not eng.calibration_is_finite():
                            eng = None
                    except HipLibraryError:
                        eng = None
                del probe
                if eng is not None:
                    warnings.warn("HAMER: this checkpoint overflows fp16 GEMM operands on the calibration crops; its activations "
                                  "were rescaled by powers of two folded into the weights (fp16 operands kept)")
                    self._engine = eng
                else:
                    warnings.warn("HAMER: this checkpoint overflows fp16 GEMM operands on the calibration crops; falling back to "
                                  "bfloat16 operands (pose / shape within ~2e-3 of the fp32 reference instead of 2e-4)")
                    self.dtype = torch.bfloat16
                    self._engine = HamerEngine(self._sd, self.mano.params, self._hc, device=device, dtype=self.dtype,
                                               token_merge=self.token_merge or None)
            self.device = device
        return self

    def _workspace(self, B: int) -> torch.Tensor:
        """The forward's scratch memory, one per HIP stream the model is called on (batches issued on different streams
        overlap on the GPU and must not share scratch); grown in steps of 64 hands."""
        key = torch.cuda.current_stream(self.device).cuda_stream
        cap, ws = self._ws.get(key, (0, None))
        if cap < B:
            cap = (B + 63) // 64 * 64
            import ctypes as C
            n = self._engine.lib.hm_hamer_workspace_bytes(C.byref(self._engine.w), cap)
            ws = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._ws[key] = (cap, ws)
        return ws

    def eval(self):
        self.training = False
        return self

    def forward_step(self, batch: Dict, train: bool = False) -> Tuple[Dict, Dict]:
        if self._engine is None:
            raise HipLibraryError("call model.to('cuda') before the first forward")
        x = batch["img"].to(self.device, torch.float32)
        B = x.shape[0]
        # The 256-row GEMM tiles (persistent kernel, in-loop residual) need B * 192 rows to be a multiple of 256, i.e. B % 4 == 0;
        # a chunk of frames yields whatever number of hands the detector found.  From 24 hands on (where those tiles are
        # chosen) the batch is padded with copies of its last crop and the extra rows are dropped again: every hand is its own
        # problem, so the real hands' results are what a batch of that size gives them.
        # (The precise route has one tile loop for every M and masks partial tiles: nothing to pad.)
        Bp = (B + 3) // 4 * 4 if B >= 24 and self.dtype != torch.float32 else B
        if Bp != B:
            x = torch.cat([x, x[-1:].expand(Bp - B, -1, -1, -1)], 0)
        o = self._engine.forward(x, workspace=self._workspace(Bp))
        if Bp != B:
            o = {k: v[:B] for k, v in o.items()}
        R = o["rotmats"]
        pred_mano_params = {"global_orient": R[:, :1], "hand_pose": R[:, 1:], "betas": o["betas"]}
        output = {
            "pred_cam": o["pred_cam"],
            "pred_mano_params": {k: v.clone() for k, v in pred_mano_params.items()},
            "pred_cam_t": o["pred_cam_t"],
            "focal_length": self.cfg.EXTRA.FOCAL_LENGTH * torch.ones(B, 2, device=self.device, dtype=torch.float32),
            "pred_keypoints_3d": o["pred_keypoints_3d"].reshape(B, -1, 3),
            "pred_vertices": o["pred_vertices"].reshape(B, -1, 3),
            "pred_keypoints_2d": o["pred_keypoints_2d"].reshape(B, -1, 2),
        }
        pred_mano_params["trans"] = o["pred_cam_t"]
        return output, pred_mano_params

    def forward(self, batch: Dict) -> Tuple[Dict, Dict]:
        return self.forward_step(batch, train=False)

    __call__ = forward


class HAMER_INFER(HAMER):
    """The reference's inference-only model class (hamer.py:468-483): ``HAMER_INFER(cfg, init_renderer, token_merge)``;
    with ``token_merge=True`` the backbone is ToMe-patched with ``r = (8, -1)`` (selective_vit_adapter.py).  Here the
    weights come in explicitly (the reference builds modules and loads a state dict afterwards)."""

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], mano: MANO, init_renderer: bool = True, token_merge: bool = False,
                 dtype=torch.float16, hamer_cfg: Optional[synth.HamerConfig] = None):
        super().__init__(cfg, state_dict, mano, dtype=dtype, hamer_cfg=hamer_cfg, token_merge=(8, -1) if token_merge else False)
