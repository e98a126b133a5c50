"""``EstimateRGB`` with the interface d_infer.py uses (reference: rootnet/Model_RGB.py:304-336,:494-498,:572-639):
``get_model()`` -> object with ``estimate_root_depth_custom(img, K, bbox) -> float`` (absolute root depth) and
``calculate_k``; and the reference's own estimator ``run(input)`` (:500-570): the SAR hand-mesh head (SAIGB + GBBMR +
SoftHeatmap) on the same ResNet-34 features, root depth from ResRootNet or a depth image, and ``post_processing`` (:428-480).
``cfg.backbone = 'convnext'`` with ``cfg.in_channels = 1024`` runs the ConvNeXt-base SAR instead (ConvNextEngine; default route only).
``run_frames`` is the batched form: all hands of several frames through one backbone, one head, one RootNet and one
post-process launch.  ``EstimateRGB(cfg, precise=True)`` (or ``cfg.precise``) runs the backbone, the depth head and the SAR
head in fp32, as the reference does, on the fp32-input MFMA: deterministic and batch-invariant."""
from __future__ import annotations

import numpy as np
import torch

from .. import lib as L
from .. import ops, synth
from .convnext_engine import ConvNextEngine
from .engine import RootNetEngine
from .preprocessing import patch_boxes, patch_transforms, process_bbox, uvd2xyz
from .sar import NV, SarHeadEngine, head_keys, sar_hand

# vis_tool.py:19-24 (joint colours, 0..1, applied to the image's channels in this order)
COLOR_HAND_JOINTS = [[1.0, 0.0, 0.0],
                     [0.0, 0.4, 0.0], [0.0, 0.6, 0.0], [0.0, 0.8, 0.0], [0.0, 1.0, 0.0],
                     [0.0, 0.0, 0.6], [0.0, 0.0, 1.0], [0.2, 0.2, 1.0], [0.4, 0.4, 1.0],
                     [0.0, 0.4, 0.4], [0.0, 0.6, 0.6], [0.0, 0.8, 0.8], [0.0, 1.0, 1.0],
                     [0.4, 0.4, 0.0], [0.6, 0.6, 0.0], [0.8, 0.8, 0.0], [1.0, 1.0, 0.0],
                     [0.4, 0.0, 0.4], [0.6, 0.0, 0.6], [0.8, 0.0, 0.8], [1.0, 0.0, 1.0]]


def draw_2d_skeleton(image: np.ndarray, pose_uv: np.ndarray) -> np.ndarray:
    """vis_tool.py:602-640 topology and colours by a plain rule (cv2 is not used, so the pixels are not cv2's): joints are
    truncated to int32; each bone (joint j to joint 0 when j % 4 == 1, else to j - 1) is a one-pixel line through the
    rounded points of max(|dx|, |dy|) + 1 evenly spaced samples; each joint a filled disc of radius 2 (dx^2 + dy^2 <= 4) in
    its colour, drawn in joint order after its bone; no anti-aliasing; pixels outside the image are skipped."""
    assert pose_uv.shape[0] == 21
    out = image.copy()
    H, W = out.shape[:2]
    pts = np.asarray(pose_uv)[:, :2].astype(np.int64).astype(np.int32)

    def put(x, y, col):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        out[y[ok], x[ok]] = col

    disc = np.array([(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if dx * dx + dy * dy <= 4])
    for j in range(21):
        col = np.round(np.array(COLOR_HAND_JOINTS[j]) * 255).astype(np.uint8)
        if j > 0:
            a, b = pts[0 if j % 4 == 1 else j - 1].astype(np.int64), pts[j].astype(np.int64)
            n = int(max(abs(b[0] - a[0]), abs(b[1] - a[1]))) + 1
            t = np.linspace(0.0, 1.0, n)
            put(np.rint(a[0] + t * (b[0] - a[0])).astype(np.int64), np.rint(a[1] + t * (b[1] - a[1])).astype(np.int64), col)
        put(pts[j, 0] + disc[:, 0].astype(np.int64), pts[j, 1] + disc[:, 1].astype(np.int64), col)
    return out


class EstimateRGB:
    def __init__(self, cfg, precise=None):
        """precise: None reads ``cfg.precise`` (default False).  True runs the fp32 route: the backbone, ResRootNet and the
        SAR head in fp32 operands; the crop, the left-hand rule, the depth-image root and the post-process are shared."""
        self.cfg = cfg
        self.mode = 'estimate'
        self.precise = bool(getattr(cfg, 'precise', False) if precise is None else precise)
        backbone = getattr(cfg, 'backbone', 'resnet34')
        if backbone == 'convnext':
            # SAR builds convnext_base only (Model_RGB.py:226-227), whose head takes cfg.in_channels = 1024 (:319)
            if getattr(cfg, 'in_channels', None) != 1024:
                raise NotImplementedError(f"EstimateRGB: backbone 'convnext' runs as ConvNeXt-base only, which needs cfg.in_channels "
                                          f"== 1024 (got {getattr(cfg, 'in_channels', None)!r})")
            if self.precise:
                raise ValueError("EstimateRGB: the fp32 route (precise=True) of the convnext backbone does not exist yet; "
                                 "precise=True runs with backbone='resnet34' only")
        elif backbone != 'resnet34':
            raise NotImplementedError(f"EstimateRGB: backbone {backbone!r} is not supported; the resnet34 and the convnext "
                                      "(ConvNeXt-base, in_channels 1024) SAR checkpoints run here")
        in_channels = 1024 if backbone == 'convnext' else 512
        ck = str(cfg.checkpoint)
        if ck.startswith("synthetic"):
            seed = int(ck.split(":")[1]) if ":" in ck else 0
            if backbone == 'convnext':
                net, root = synth.convnext_state_dict(seed), synth.convnext_rootnet_state_dict(seed)
            else:
                net, root = synth.rootnet_state_dict(seed)
            net = {**net, **synth.sar_head_state_dict(seed, in_channels)}
        else:
            from ..utils.checkpoint import load_checkpoint
            checkpoint = load_checkpoint(ck)                       # FileNotFoundError when missing
            net = checkpoint['net'] if 'net' in checkpoint else checkpoint['network']      # Model_RGB.py:321-324
            root = checkpoint.get('rootnet')                       # None: run() serves root depth 0 (:533)
        self.device = torch.device(cfg.device if torch.cuda.is_available() else 'cpu')
        if self.device.type != 'cuda':
            raise L.HipLibraryError("EstimateRGB runs on an MI355X only: the HIP hot path has no CPU fallback")
        if backbone == 'convnext':
            self.engine = ConvNextEngine(net, root, device=self.device, dtype=torch.float16)
        else:
            self.engine = RootNetEngine(net, root, device=self.device, dtype=torch.float32 if self.precise else torch.float16)
        self.rootnet = self.engine if root is not None else None
        self.head = (SarHeadEngine(net, device=self.device, precise=self.precise, in_channels=in_channels)
                     if all(k in net for k in head_keys()) else None)
        self.mean = 255.0 * np.array([0.485, 0.456, 0.406])
        self.std = 255.0 * np.array([0.229, 0.224, 0.225])

    def _k_host(self, bbox, fx, fy):
        area = bbox[-1] * bbox[-2]
        real_area = torch.tensor(self.cfg.bbox_real[0] * self.cfg.bbox_real[1])
        return torch.sqrt(real_area * fx * fy / (area)).unsqueeze(0)

    def calculate_k(self, bbox, fx, fy):
        """Model_RGB.py:494-498: sqrt(real_area * fx * fy / bbox_area), shape (1,)."""
        return self._k_host(bbox, fx, fy).to(self.device)

    def patch(self, img: np.ndarray, bbox_processed) -> torch.Tensor:
        """generate_patch_image + BGR->RGB + ToTensor + Normalize (:596-610) for one box, on the GPU."""
        frame = torch.from_numpy(np.ascontiguousarray(img)).to(self.device)
        cx, cy = float(bbox_processed[0] + 0.5 * bbox_processed[2]), float(bbox_processed[1] + 0.5 * bbox_processed[3])
        rec = ops.crop_boxes([(cx, cy, float(bbox_processed[2]), False)]).to(self.device)
        return ops.crop_batch(frame, rec, self.mean, self.std)

    @torch.no_grad()
    def estimate_root_depth_custom(self, img, K, bbox):
        """Model_RGB.py:572-639.  img HxWx3 uint8 BGR, K 3x3, bbox [x1, y1, x2, y2] -> root depth (float)."""
        if self.rootnet is None:
            raise RuntimeError("RootNet is not loaded in the checkpoint!")          # :586-587
        x1, y1, x2, y2 = bbox
        height, width = img.shape[:2]
        bbox_processed = process_bbox([x1, y1, x2 - x1, y2 - y1], width, height, self.cfg.input_img_shape, 1.5)
        if bbox_processed is None:
            raise ValueError("empty bounding box")
        fx, fy = (K[0, 0], K[1, 1]) if isinstance(K, np.ndarray) else (K[0][0], K[1][1])
        k_value = self.calculate_k(bbox_processed, float(fx), float(fy))
        depth = self.engine.forward(self.patch(img, bbox_processed), k_value)
        return depth.item()


    # -------------------------------------------------------------------------------- batched form (d_infer's folder driver)
    def valid_boxes(self, dets, width, height):
        """Which detections [[label, [x1, y1, x2, y2]], ...] of a width x height frame have a RootNet patch at all (the ones
        estimate_root_depth_custom would raise on -- the reference's per-hand try/except skips those hands)."""
        if not dets:
            return np.zeros(0, dtype=bool)
        xywh = np.array([[d[1][0], d[1][1], d[1][2] - d[1][0], d[1][3] - d[1][1]] for d in dets], dtype=np.float64)
        return patch_boxes(xywh, width, height, self.cfg.input_img_shape, 1.5)[1]

    @torch.no_grad()
    def estimate_root_depths_frames(self, frames, K, dets_lists) -> torch.Tensor:
        """estimate_root_depth_custom for ALL hands of several device-resident frames ((H,W,3) uint8 BGR tensors) in one
        RootNet forward: one crop launch per frame into one batch tensor, one pass of the backbone.  Per hand the same
        box arithmetic, the same crop and the same k as the one-hand call, so the depths are the same numbers.  Every
        detection must have a patch (filter with valid_boxes first).  Returns (n,) fp32 on the device, hands in
        ``dets_lists`` order."""
        if self.rootnet is None:
            raise RuntimeError("RootNet is not loaded in the checkpoint!")
        fx, fy = (K[0, 0], K[1, 1]) if isinstance(K, np.ndarray) else (K[0][0], K[1][1])
        P = int(self.cfg.input_img_shape[0])
        recs, kvs, counts = [], [], []
        for fr, dets in zip(frames, dets_lists):
            height, width = int(fr.shape[0]), int(fr.shape[1])
            for _, (x1, y1, x2, y2) in dets:
                bp = process_bbox([x1, y1, x2 - x1, y2 - y1], width, height, self.cfg.input_img_shape, 1.5)
                if bp is None:
                    raise ValueError("empty bounding box")
                recs.append((float(bp[0] + 0.5 * bp[2]), float(bp[1] + 0.5 * bp[3]), float(bp[2]), False))
                kvs.append(self._k_host(bp, float(fx), float(fy)))          # host arithmetic (correctly rounded ops: the same bits), one upload
            counts.append(len(dets))
        n = len(recs)
        if n == 0:
            return torch.empty(0, device=self.device)
        rec = ops.crop_boxes(recs, P).to(self.device)
        rsz = rec.numel() // n
        img = torch.empty(n, 3, P, P, device=self.device, dtype=torch.float32)
        off = 0
        for fr, k in zip(frames, counts):
            if k:
                ops.crop_batch(fr, rec[off * rsz:(off + k) * rsz], self.mean, self.std, P, out=img[off:off + k])
                off += k
        return self.engine.forward(img, torch.cat(kvs))

    # -------------------------------------------------------------------------------- SAR mesh head (run, :500-570)
    def _require_head(self):
        if self.head is None:
            raise RuntimeError("the checkpoint holds no SAR head (head.* keys): EstimateRGB.run needs the full SAR model")

    def _sar_patches(self, frames, boxes, flips, P):
        """One (B, 3, P, P) fp32 batch: for each hand (frame index, bbox_processed, flip) the patch of
        generate_patch_image (:517-521).  A left hand's patch is cut, unflipped, from the MIRRORED frame at
        bb_c_x = W - bb_c_x - 1, exactly the reference's rule (the crop kernel's own flip mirrors the patch after the crop,
        HaMeR's rule, which samples one patch pixel further along x)."""
        n = len(boxes)
        img = torch.empty(n, 3, P, P, device=self.device, dtype=torch.float32)
        raw = torch.empty(n, 3, P, P, device=self.device, dtype=torch.float32)
        mirrored = {}
        for i, ((fi, bp), flip) in enumerate(zip(boxes, flips)):
            fr = frames[fi]
            W = int(fr.shape[1])
            cx, cy = float(bp[0] + 0.5 * bp[2]), float(bp[1] + 0.5 * bp[3])
            if flip:
                if fi not in mirrored:
                    mirrored[fi] = torch.flip(fr, dims=[1]).contiguous()
                fr, cx = mirrored[fi], W - cx - 1
            rec = ops.crop_boxes([(cx, cy, float(bp[2]), False)], P).to(self.device)
            ops.crop_batch(fr, rec, self.mean, self.std, P, out=img[i:i + 1])
            ops.crop_batch(fr, rec, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), P, out=raw[i:i + 1])
        return img, raw

    @torch.no_grad()
    def _sar_batch(self, frames, hands, K, depth=None, depth_wh=(0, 0)):
        """hands: [(frame index, bbox_processed, do_flip, depth_offset)] -> (uvd, xyz (n, 799, 3) device, raw patches,
        (img2bb, bb2img) per hand, head coords (n, 799, 3))."""
        self._require_head()
        P = int(self.cfg.input_img_shape[0])
        fx, fy = float(K[0][0]), float(K[1][1])
        img, raw = self._sar_patches(frames, [(h[0], h[1]) for h in hands], [h[2] for h in hands], P)
        feats = self.engine.features(img)
        coords = self.head.forward(feats)
        root = None
        if self.rootnet is not None and any(h[3] < 0 for h in hands):
            kv = torch.cat([self._k_host(h[1], fx, fy) for h in hands]).to(self.device, torch.float32)
            root = self.engine.depth_of(feats, kv)
        recs, trans = [], []
        for fi, bp, flip, doff in hands:
            H, W = int(frames[fi].shape[0]), int(frames[fi].shape[1])
            img2bb, bb2img = patch_transforms(bp, flip, W, self.cfg.input_img_shape)
            trans.append((img2bb, bb2img))
            recs.append(sar_hand(bb2img, K, W, H, flip, self.cfg.depth_box, doff, depth_wh))
        uvd, xyz = self.head.postprocess(coords, recs, root, depth, P)
        return uvd, xyz, raw, trans, coords

    def _processed_box(self, bbox, width, height):
        x1, y1, x2, y2 = bbox
        bp = process_bbox([x1, y1, x2 - x1, y2 - y1], width, height, self.cfg.input_img_shape, 1.5)
        if bp is None:
            raise ValueError("empty bounding box")
        return bp

    def camera_K(self):
        fx, fy, fu, fv = self.cfg.cam_para
        return np.array([[fx, 0, fu], [0, fy, fv], [0, 0, 1]])

    @torch.no_grad()
    def run(self, input):
        """Model_RGB.py:500-570.  input: [{'rgb': HxWx3 uint8 BGR, 'rgb_bbox': [x1, y1, x2, y2], 'hand_type': 'left' |
        'right'[, 'depth': HxW depth in millimetres]}] (the first entry is used) -> (meta_info_output, output) with output =
        {pose_uvd (21, 3), mesh_uvd (778, 3), pose_xyz (21, 3), mesh_xyz (778, 3)} float32 in frame pixels / metres.
        The camera is cfg.cam_para.  Root depth: the depth image when given, else ResRootNet on the same features, else 0."""
        inp = input[0]
        img_rgb, bbox, hand_type = inp['rgb'], inp['rgb_bbox'], inp['hand_type']
        do_flip = hand_type == "left"
        height, width = img_rgb.shape[:-1]
        bp = self._processed_box(bbox, width, height)
        K = self.camera_K()
        frame = torch.from_numpy(np.ascontiguousarray(img_rgb)).to(self.device)
        depth, doff, dwh = None, -1, (0, 0)
        if inp.get('depth') is not None:
            d = np.asarray(inp['depth'])
            depth = torch.from_numpy(d.astype(np.float32) / 1000.).to(self.device).contiguous()
            doff, dwh = 0, (d.shape[1], d.shape[0])
        uvd, xyz, raw, trans, coords = self._sar_batch([frame], [(0, bp, do_flip, doff)], K, depth, dwh)
        uvd, xyz = uvd[0].cpu().numpy(), xyz[0].cpu().numpy()
        img2bb = trans[0][0]
        output = {'pose_uvd': uvd[NV:], 'mesh_uvd': uvd[:NV], 'pose_xyz': xyz[NV:], 'mesh_xyz': xyz[:NV]}
        crop = self._crop_u8(raw[0])
        P = np.float32(self.cfg.input_img_shape[0])
        pose_crop_uv = (coords[0, NV:, :2].cpu().numpy() + np.float32(0.5)) * P           # coord_uvd_crop (:438)
        meta = self._meta(crop, pose_crop_uv, output['pose_xyz'], img2bb)
        return meta, output

    def _crop_u8(self, raw: torch.Tensor) -> np.ndarray:
        """The u8 BGR patch (generate_patch_image's img_patch) of a raw (3, P, P) RGB crop."""
        return raw.flip(0).permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8).cpu().numpy()

    def _meta(self, crop, pose_crop_uv, pose_xyz, img2bb):
        """meta_info_output of post_processing (:467-478)."""
        center = np.mean(pose_xyz, axis=0, keepdims=True)
        M = torch.cat((torch.tensor(img2bb), torch.tensor([[0, 0, 1]])), dim=0).unsqueeze(0)
        return {'crop_img_rgb': crop, 'crop_img_d': None, 'pose_img_rgb': draw_2d_skeleton(crop, pose_crop_uv),
                'pose_img_d': None, 'joint_xyz_world': pose_xyz, 'cam_para': self.cfg.cam_para,
                'center': torch.from_numpy(center), 'cube': self.cfg.depth_box * 1000, 'M': M, 'img2bb_trans': img2bb}

    def post_processing(self, outs, meta_info, img_width, do_flip=False):
        """Model_RGB.py:428-480 on the host (the reference's signature; run() does the same arithmetic in one GPU launch):
        outs {'coords': (B, 799, 3)}, meta_info {'crop_img', 'root_depth', 'bb2img_trans', 'img2bb_trans', 'K'} ->
        (eval_result {pose_uvd, mesh_uvd, pose_xyz, mesh_xyz: lists per hand}, meta_info_output of the last hand)."""
        crop_img = meta_info['crop_img']
        coords_uvd = outs['coords']
        eval_result = {'pose_uvd': list(), 'mesh_uvd': list(), 'pose_xyz': list(), 'mesh_xyz': list()}
        meta_info_output = None
        for i in range(coords_uvd.shape[0]):
            c, root_depth, bb2img, K = coords_uvd[i], meta_info['root_depth'][i], meta_info['bb2img_trans'][i], meta_info['K'][i]
            c[:, 2] = c[:, 2] * self.cfg.depth_box + root_depth
            c[:, :2] = (c[:, :2] + 0.5) * self.cfg.input_img_shape[0]
            full = c.copy()
            uv1 = np.concatenate((full[:, :2], np.ones_like(full[:, :1])), 1)
            full[:, :2] = np.dot(bb2img, uv1.transpose(1, 0)).transpose(1, 0)[:, :2]
            if do_flip:
                full[:, 0] = img_width - full[:, 0] - 1
            eval_result['pose_uvd'].append(full[NV:])
            eval_result['mesh_uvd'].append(full[:NV])
            xyz = uvd2xyz(full, K)
            eval_result['pose_xyz'].append(xyz[NV:])
            eval_result['mesh_xyz'].append(xyz[:NV])
            meta_info_output = self._meta(crop_img[0], c[NV:, :2], xyz[NV:], meta_info['img2bb_trans'][0])
        return eval_result, meta_info_output

    def convert2origin_pixel(self, uvd, inv_trans):
        """Model_RGB.py:482-492: uvd (B, J, 3) normalised, inv_trans (B or 1, 2, 3) bb2img -> (B, J, 2) frame pixels."""
        uv = (uvd[:, :, :2] + 0.5) * self.cfg.input_img_shape[1]
        uv1 = torch.cat((uv[:, :, :2], torch.ones_like(uvd[:, :, :1])), dim=2)
        return (inv_trans @ uv1.transpose(-1, -2)).transpose(-1, -2)

    @torch.no_grad()
    def run_frames(self, frames, K, dets_lists, draw=False):
        """run() for ALL hands of several device-resident frames ((H, W, 3) uint8 BGR tensors): one backbone pass, one head,
        one RootNet and one post-process launch.  dets_lists: per frame [[hand_type, [x1, y1, x2, y2]], ...] (every box must
        have a patch: filter with valid_boxes).  K: 3x3 camera.  Returns {pose_uvd (n, 21, 3), mesh_uvd (n, 778, 3),
        pose_xyz, mesh_xyz} fp32 device tensors, hands in dets_lists order; the same numbers as run() hand by hand.
        draw=True adds run()'s two images per hand, made on the device: crop_img_rgb (n, P, P, 3) uint8, the patch by
        _crop_u8's arithmetic, and pose_img_rgb, the patch with the skeleton drawn by hm_skeleton_overlay at
        (coords[:, NV:, :2] + 0.5) * P (render.skeleton_frames, style 'sar': the bytes of draw_2d_skeleton)."""
        P = int(self.cfg.input_img_shape[0])
        hands = []
        for fi, (fr, dets) in enumerate(zip(frames, dets_lists)):
            for label, box in dets:
                hands.append((fi, self._processed_box(box, int(fr.shape[1]), int(fr.shape[0])), label == "left", -1))
        if not hands:
            e = torch.empty(0, 21, 3, device=self.device)
            res = {'pose_uvd': e, 'mesh_uvd': torch.empty(0, NV, 3, device=self.device), 'pose_xyz': e.clone(),
                   'mesh_xyz': torch.empty(0, NV, 3, device=self.device)}
            if draw:
                res['crop_img_rgb'] = torch.empty(0, P, P, 3, dtype=torch.uint8, device=self.device)
                res['pose_img_rgb'] = res['crop_img_rgb'].clone()
            return res
        uvd, xyz, raw, _, coords = self._sar_batch(frames, hands, K)
        res = {'pose_uvd': uvd[:, NV:], 'mesh_uvd': uvd[:, :NV], 'pose_xyz': xyz[:, NV:], 'mesh_xyz': xyz[:, :NV]}
        if draw:
            from ..render import skeleton_frames
            crop = raw.flip(1).permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous()     # _crop_u8, batched
            pose_crop_uv = (coords[:, NV:, :2].to(torch.float32) + 0.5) * float(P)                       # coord_uvd_crop (:438)
            res['crop_img_rgb'] = crop
            res['pose_img_rgb'] = skeleton_frames(crop, pose_crop_uv, range(len(hands)), style='sar')
        return res


def get_model():
    from .sar_config_stage_1 import rgb_opt
    return EstimateRGB(rgb_opt)
