"""ConvNeXt-base as the reference's SAR builds it (rootnet/Model_RGB.py:226-227: ``convnext_base(pretrained=False, in_22k=True,
num_classes=21841)``, rootnet/convnext.py:66-114, :185-187): the shapes and the state-dict keys under ``backbone.``.  The
classifier ``head`` (21841 x 1024) is part of the state dict and is never used by ``forward`` (:108-114): no key of it is mapped."""
from __future__ import annotations

from typing import Dict, List, Tuple

DEPTHS = (3, 3, 27, 3)
DIMS = (128, 256, 512, 1024)
LN_EPS = 1e-6
PREFIX = "backbone."
NUM_CLASSES = 21841
UNUSED = ("head.weight", "head.bias")          # under PREFIX: in the checkpoint, never read, never uploaded
GFLOP_PER_HAND = 40.1                          # 256 x 256 patch: 38.7 pointwise, 0.8 downsample, 0.6 depthwise


def blocks() -> List[Tuple[str, int, int]]:
    """(key prefix, stage, dim) of the 36 blocks in forward order."""
    return [(f"{PREFIX}stages.{i}.{j}.", i, DIMS[i]) for i in range(4) for j in range(DEPTHS[i])]


def key_shapes() -> Dict[str, tuple]:
    """Every key of the reference's ``backbone.*`` state dict that the forward reads -> its shape."""
    ks: Dict[str, tuple] = {}
    d = PREFIX + "downsample_layers."
    ks[d + "0.0.weight"], ks[d + "0.0.bias"] = (DIMS[0], 3, 4, 4), (DIMS[0],)          # stem: conv, then LayerNorm
    ks[d + "0.1.weight"], ks[d + "0.1.bias"] = (DIMS[0],), (DIMS[0],)
    for i in range(1, 4):                                                              # LayerNorm, then conv
        ks[d + f"{i}.0.weight"], ks[d + f"{i}.0.bias"] = (DIMS[i - 1],), (DIMS[i - 1],)
        ks[d + f"{i}.1.weight"], ks[d + f"{i}.1.bias"] = (DIMS[i], DIMS[i - 1], 2, 2), (DIMS[i],)
    for pre, _, c in blocks():
        ks[pre + "gamma"] = (c,)
        ks[pre + "dwconv.weight"], ks[pre + "dwconv.bias"] = (c, 1, 7, 7), (c,)
        ks[pre + "norm.weight"], ks[pre + "norm.bias"] = (c,), (c,)
        ks[pre + "pwconv1.weight"], ks[pre + "pwconv1.bias"] = (4 * c, c), (4 * c,)
        ks[pre + "pwconv2.weight"], ks[pre + "pwconv2.bias"] = (c, 4 * c), (c,)
    ks[PREFIX + "norm.weight"], ks[PREFIX + "norm.bias"] = (DIMS[3],), (DIMS[3],)
    return ks


def is_convnext(net_sd) -> bool:
    return PREFIX + "downsample_layers.0.0.weight" in net_sd
