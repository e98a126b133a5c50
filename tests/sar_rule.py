"""fp32 restatement of the SAR hand-mesh head and of EstimateRGB.run's post-processing (rootnet/Model_RGB.py:76-177,
:428-480, :500-570; preprocessing.py:11-17, :101-150), the oracle of tests/test_gpu_sar.py.  torch-CPU / numpy only; the
committed fixture tests/golden/sar_head.npz (written from the reference's own modules) pins it."""
import numpy as np
import torch
import torch.nn.functional as F

NV, NJ, HM = 778, 21, 32
NT = NV + NJ


def laplacian(adj):
    """GraphConv.laplacian (:104-108): 1 / (rowsum + 1e-5) * A, fp32."""
    d = torch.sum(adj, 1, keepdim=True) + 1e-5
    return 1 / d * adj


def saigb(sd, feat):
    """SAIGB.forward (:131-136): feat (B, 512, 8, 8) -> init graph (B, 778, 515)."""
    y = F.leaky_relu(F.conv2d(feat, sd["head.saigb.group.0.weight"], sd["head.saigb.group.0.bias"]), 0.1)
    f = y.view(-1, NV, 512)
    return torch.cat((f, sd["head.saigb.template"].repeat(feat.shape[0], 1, 1)), dim=2)


def graph_conv(sd, pre, x):
    return F.linear(torch.matmul(laplacian(sd[pre + "adj"]), x), sd[pre + "fc.weight"], sd[pre + "fc.bias"])


def branch(sd, name, x):
    """reg_xy / reg_z (:146-157), eval mode (Dropout is the identity)."""
    pre = f"head.gbbmr.{name}."
    return graph_conv(sd, pre + "3.", F.leaky_relu(graph_conv(sd, pre + "0.", x), 0.1))


@torch.no_grad()
def head(sd, feat, return_heatmaps=False):
    """SARhead.forward (:213-222): feat (B, 512, 8, 8) fp32 -> coords (B, 799, 3) fp32 (xy normalised, z relative)."""
    sd = {k: v.float() for k, v in sd.items()}
    g = saigb(sd, feat.float())
    return tail(sd, branch(sd, "reg_xy", g), branch(sd, "reg_z", g), return_heatmaps)


@torch.no_grad()
def tail(sd, logits_xy, logits_z, return_heatmaps=False):
    """GBBMR.forward after the two branches (:163-176): second-layer logits (B, 778, 1024) each -> coords (B, 799, 3)."""
    hm_xy = logits_xy.float().reshape(-1, NV, HM, HM)
    hm_z = logits_z.float().reshape(-1, NV, HM, HM)
    sd = {k: v.float() for k, v in sd.items() if k.startswith("head.gbbmr.")}
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
    return (coords, p) if return_heatmaps else coords


def patch_trans(bbox, do_flip, img_width, P=256):
    """generate_patch_image's (trans, inv_trans) for rot 0, scale 1 (preprocessing.py:40-150): cv2.getAffineTransform of the
    three float32 control points, solved in closed form in double, returned as float32 (img2bb, bb2img)."""
    cx, cy = float(bbox[0] + 0.5 * bbox[2]), float(bbox[1] + 0.5 * bbox[3])
    if do_flip:
        cx = img_width - cx - 1
    c = np.array([cx, cy], np.float32)
    down = c + np.array([0, bbox[3] * 0.5], np.float32)
    right = c + np.array([bbox[2] * 0.5, 0], np.float32)
    ax = (float(right[0]) - float(c[0])) / (P * 0.5)          # d src / d dst
    by = (float(down[1]) - float(c[1])) / (P * 0.5)
    inv = np.array([[ax, 0.0, float(c[0]) - ax * P * 0.5], [0.0, by, float(c[1]) - by * P * 0.5]])
    fwd = np.array([[1 / ax, 0.0, P * 0.5 - float(c[0]) / ax], [0.0, 1 / by, P * 0.5 - float(c[1]) / by]])
    return fwd.astype(np.float32), inv.astype(np.float32)


def root_from_depth(coords, bb2img, depth_mm, width, height, P=256):
    """run's depth-image root (:538-546): convert2origin_pixel of row 778 (NOT un-flipped for a left hand), normalised by
    the integer halves of the RGB size, grid_sample (bilinear, zeros, align_corners False) of depth / 1000."""
    d = torch.from_numpy(np.asarray(depth_mm).astype(np.float32) / 1000.)[None, None]
    uvd = torch.from_numpy(np.asarray(coords, np.float32)[None, NV:NV + 1])
    uv = (uvd[:, :, :2] + 0.5) * P
    uv1 = torch.cat((uv, torch.ones_like(uvd[:, :, :1])), dim=2)
    uv = (torch.from_numpy(bb2img) @ uv1.transpose(-1, -2)).transpose(-1, -2)
    g = uv.clone()
    g[:, :, 0] = g[:, :, 0] / (width // 2) - 1
    g[:, :, 1] = g[:, :, 1] / (height // 2) - 1
    return np.float32(F.grid_sample(d, g[:, None], align_corners=False)[:, 0, 0].reshape(-1)[0].item())


def uvd2xyz(uvd, K):
    fx, fy, fu, fv = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    xyz = np.zeros_like(uvd, np.float32)
    xyz[:, 0] = (uvd[:, 0] - fu) * uvd[:, 2] / fx
    xyz[:, 1] = (uvd[:, 1] - fv) * uvd[:, 2] / fy
    xyz[:, 2] = uvd[:, 2]
    return xyz


def post_process(coords, root, bb2img, K, img_width, do_flip, depth_box=0.3, P=256):
    """post_processing for one hand (:428-465): coords (799, 3) -> {pose_uvd, mesh_uvd, pose_xyz, mesh_xyz} float32."""
    c = np.array(coords, np.float32)
    c[:, 2] = c[:, 2] * depth_box + np.float32(root)
    c[:, :2] = (c[:, :2] + 0.5) * P
    full = c.copy()
    uv1 = np.concatenate((full[:, :2], np.ones_like(full[:, :1])), 1)
    full[:, :2] = np.dot(bb2img, uv1.transpose(1, 0)).transpose(1, 0)[:, :2]
    if do_flip:
        full[:, 0] = img_width - full[:, 0] - 1
    xyz = uvd2xyz(full, np.asarray(K, np.float64))
    return {"pose_uvd": full[NV:], "mesh_uvd": full[:NV], "pose_xyz": xyz[NV:], "mesh_xyz": xyz[:NV]}
