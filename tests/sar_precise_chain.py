"""The whole SAR / RootNet chain in fp64 on the CPU, the oracle of tests/test_gpu_sar_precise.py (the fp32 route of
EstimateRGB): the ResNet-34 backbone and ResRootNet of oracle/rootnet_ref on double tensors, and the SAR head
(rootnet/Model_RGB.py:76-222) restated in double.  tests/sar_rule.head casts to float, so only its dtype-agnostic pieces
(laplacian, patch_trans, post_process, uvd2xyz) are reused; tests/test_sar_precise_host.py pins head() here to
sar_rule.head on the committed fixture tests/golden/sar_head.npz, so it inherits that file's pin to the reference."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sar_rule as R  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import rootnet_ref as RR  # noqa: E402

NV, NJ, HM, NT = R.NV, R.NJ, R.HM, R.NT


def _d(sd):
    return {k: v.double() for k, v in sd.items()}


@torch.no_grad()
def backbone(net_sd, img):
    """SARresnet34.forward in fp64: img (B, 3, 256, 256) -> (B, 512, 8, 8) double."""
    return RR.backbone(_d(net_sd), img.double())


@torch.no_grad()
def root_depth(root_sd, feat, k_value):
    """ResRootNet.forward_coord in fp64 -> (B,) double."""
    return RR.root_depth(_d(root_sd), feat.double(), torch.as_tensor(k_value, dtype=torch.float64)).reshape(-1)


def _graph_conv(sd, pre, x):
    return F.linear(torch.matmul(R.laplacian(sd[pre + "adj"]), x), sd[pre + "fc.weight"], sd[pre + "fc.bias"])


def _branch(sd, name, x):
    pre = f"head.gbbmr.{name}."
    return _graph_conv(sd, pre + "3.", F.leaky_relu(_graph_conv(sd, pre + "0.", x), 0.1))


@torch.no_grad()
def head(sd, feat):
    """SARhead.forward in fp64: feat (B, 512, 8, 8) -> coords (B, 799, 3) double (xy normalised, z relative)."""
    sd = _d({k: v for k, v in sd.items() if k.startswith("head.")})
    feat = feat.double()
    y = F.leaky_relu(F.conv2d(feat, sd["head.saigb.group.0.weight"], sd["head.saigb.group.0.bias"]), 0.1)
    g = torch.cat((y.reshape(-1, NV, 512), sd["head.saigb.template"].repeat(feat.shape[0], 1, 1)), dim=2)
    hm_xy = _branch(sd, "reg_xy", g).reshape(-1, NV, HM, HM)
    hm_z = _branch(sd, "reg_z", g).reshape(-1, NV, HM, HM)
    j_xy = F.linear(hm_xy.transpose(1, 3), sd["head.gbbmr.mesh2pose_hm.weight"], sd["head.gbbmr.mesh2pose_hm.bias"]).transpose(1, 3)
    j_z = F.linear(hm_z.transpose(1, 3), sd["head.gbbmr.mesh2pose_dm.weight"], sd["head.gbbmr.mesh2pose_dm.bias"]).transpose(1, 3)
    hxy, hz = torch.cat((hm_xy, j_xy), 1), torch.cat((hm_z, j_z), 1)
    B = hxy.shape[0]
    s = hxy * sd["head.gbbmr.soft_heatmap.beta.weight"].view(1, NT, 1, 1)
    p = F.softmax(s.view(B, NT, HM * HM), dim=2).view(B, NT, HM, HM)
    x = torch.sum((p * sd["head.gbbmr.soft_heatmap.wx"]).view(B, NT, -1), dim=2)
    y = torch.sum((p * sd["head.gbbmr.soft_heatmap.wy"]).view(B, NT, -1), dim=2)
    z = torch.sum((p * hz).view(B, NT, -1), dim=2, keepdim=True)
    coords = torch.cat((torch.stack([x, y], dim=2), z), 2)
    coords[:, :, :2] = coords[:, :, :2] / (HM // 2) - 1
    return coords


def run(sd, root_sd, img, bbox_processed, do_flip, K, img_width, depth_box=0.3, root=None):
    """EstimateRGB.run after the crop, in fp64 up to the post-process: img (1, 3, 256, 256) the patch the GPU cut; root: the
    depth-image root (R.root_from_depth) or None for ResRootNet's.  Returns (post_process dict, coords (799, 3) double,
    root depth)."""
    feat = backbone(sd, img)
    coords = head(sd, feat)[0]
    if root is None:
        k = RR.calculate_k(bbox_processed, float(K[0][0]), float(K[1][1]))
        root = float(root_depth(root_sd, feat, [k])[0])
    _, bb2img = R.patch_trans(bbox_processed, do_flip, img_width)
    return R.post_process(coords.numpy(), np.float32(root), bb2img, K, img_width, do_flip, depth_box), coords, root
