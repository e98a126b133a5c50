"""``d_infer.py`` of the reference is ``infer.py`` plus a root depth from RootNet fed to the camera maths as
``depth_refine`` (reference: hamer/d_infer.py:21,:355,:438-440,:1223-1318 -> renderer.py:47-52): per detected hand
``depth = sar.estimate_root_depth_custom(image, k_real, bbox)`` then ``estimate_from_rgb(image, [bbox], k_real,
depth_refine=depth)``.  Everything else (``hamer_inference``, savers, CLI) is infer.py's."""
import argparse
import os

import numpy as np

from .infer import *  # noqa: F401,F403
from .infer import (FRAMES_PER_STEP, _default_models, _detection_list, _imread_bgr, _list_images, _antialias_args, _precise_hamer_args, _tta_args, apply_tta_args, _record_from, _render_args, _depth_args, depth_args, refine_records, _mask_fit_args, mask_fit_records, _visibility_args, visibility_records, _penetration_args, penetration_records, _smooth_args, smooth_args, smooth_records, render_keypoint_args, apply_antialias_args, apply_precise_args, hamer_inference,  # noqa: F401
                    hamer_opt, hand_record, iter_folder_results, load_intrinsics, reconstruct_and_save_obj_with_wrapper)
from .rootnet.Model_RGB import get_model  # noqa: F401


def process_batch_manopara(input_folder, output_folder, k_real=None, hamer=None, detector=None, sar=None,
                           frames_per_step: int = FRAMES_PER_STEP, rank=None, world=None, **pipeline):
    """d_infer.py:1223-1318: as infer.py's, with the RootNet depth per hand.  ``k_real`` is required here (the depth is
    metric only with real intrinsics; the reference passes its camera file).  The reference runs one RootNet and one HaMeR
    forward per hand; here the folder goes through infer.py's pipeline with ONE RootNet forward and ONE HaMeR forward per
    batch of hands -- each hand's camera translation still uses its own depth (``depth_refine`` is a per-hand vector in the
    camera step), and the numbers are those of the one-hand calls.  Rank sharding as infer.process_batch_manopara."""
    from .infer import _rank_world
    os.makedirs(output_folder, exist_ok=True)
    if k_real is None:
        raise ValueError("d_infer needs camera intrinsics (k_real)")
    hamer, detector = _default_models(hamer, detector)
    if sar is None:
        sar = get_model()
    rank, world = _rank_world(rank, world)
    stats = {}
    for img_path, detection_list, hands in iter_folder_results(_list_images(input_folder), hamer, detector, k_real, frames_per_step,
                                                               depth_model=sar, rank=rank, world=world, stats=stats, **pipeline):
        file_name = os.path.splitext(os.path.basename(img_path))[0]
        image_results = {'left': None, 'right': None}
        for i, bbox in enumerate(detection_list):
            image_results[bbox[0]] = _record_from(hands, i, bbox[0] == 'right')
        np.save(os.path.join(output_folder, f"{file_name}.npy"), image_results)
    return stats


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="YOLOv7 -> RootNet depth + HaMeR -> MANO parameters (.npy per image)")
    ap.add_argument('--input', type=str, required=True)
    ap.add_argument('--output', type=str, required=True)
    ap.add_argument('--intrinsics', type=str, required=True, help="3x3 camera matrix txt")
    ap.add_argument('--obj', type=str, default=None, help="also reconstruct OBJ meshes into this folder")
    ap.add_argument('--precise-detector', action='store_true',
                    help="run YOLOv7 in fp32 (the reference's CPU branch) instead of fp16: its boxes, at about twice the detector time")
    ap.add_argument('--precise-rootnet', action='store_true',
                    help="run the RootNet backbone and depth head in fp32, as the reference does, instead of fp16 (DESIGN §9)")
    ap.add_argument('--rootnet-backbone', choices=('resnet34', 'convnext'), default=None,
                    help="the SAR backbone of the RootNet checkpoint (rgb_opt.backbone / rgb_opt.in_channels: 512 / 1024); "
                         "default: the config's (resnet34)")
    _tta_args(ap)
    _precise_hamer_args(ap)
    _antialias_args(ap)
    _render_args(ap)
    ap.add_argument('--masks', type=str, default=None, metavar="DIR",
                    help="label masks DIR/<name>.npy for --mask-fit (the detector still finds the hands)")
    ap.add_argument('--mask-label', type=int, default=3, help="with --masks: the label of the hands' pixels (default 3, the reference's)")
    _mask_fit_args(ap)
    _depth_args(ap)
    _visibility_args(ap)
    _penetration_args(ap)
    _smooth_args(ap)
    return ap


def apply_rootnet_backbone(args) -> None:
    """``--rootnet-backbone`` -> ``rgb_opt.backbone`` and the ``rgb_opt.in_channels`` that goes with it."""
    if getattr(args, "rootnet_backbone", None):
        from .rootnet.sar_config_stage_1 import rgb_opt
        rgb_opt.backbone = args.rootnet_backbone
        rgb_opt.in_channels = {'resnet34': 512, 'convnext': 1024}[args.rootnet_backbone]


def main(argv=None):
    """``python -m hamer_yolo_amd.d_infer --input <RGB_dir> --output <out_dir> --intrinsics <cam_K.txt>``."""
    ap = _parser()
    args = ap.parse_args(argv)
    keypoint_kw = render_keypoint_args(ap, args)
    depth_args(ap, args)
    smooth_args(ap, args)
    if not args.masks and (args.mask_fit != "none" or args.mask_label != 3):
        ap.error("--mask-fit / --mask-label need --masks DIR")
    if not 1 <= args.mask_label <= 255:
        ap.error("--mask-label must be in 1..255")
    apply_precise_args(args)
    apply_antialias_args(args)
    apply_tta_args(args)
    apply_rootnet_backbone(args)
    k_real = load_intrinsics(args.intrinsics)
    hamer = hamer_inference(hamer_opt)
    process_batch_manopara(args.input, args.output, k_real, hamer=hamer)
    if args.masks and args.mask_fit == "contour":                  # before the depth step: that one starts from the fitted records
        from .infer import _rank_world
        mask_fit_records(args, hamer, *_rank_world(None, None))
    if args.depth_maps:
        from .infer import _rank_world
        refine_records(args, hamer, *_rank_world(None, None))
    if args.penetration or args.resolve_penetration:               # after the refinements: they move the hands
        from .infer import _rank_world
        penetration_records(args, hamer, *_rank_world(None, None))
    if args.smooth_tracks:                                         # after every step that moves a hand, before every step that reads one
        from .infer import _rank_world
        smooth_records(args, hamer, *_rank_world(None, None))
    if args.visibility:
        from .infer import _rank_world
        visibility_records(args, hamer, *_rank_world(None, None))
    if args.obj:
        reconstruct_and_save_obj_with_wrapper(args.output, args.obj, hamer)
    if args.render:
        from .infer import _rank_world
        from .render import render_folder
        rank, world = _rank_world(None, None)
        render_folder(args.input, args.output, args.render, hamer, k_real, style=args.render_style, rank=rank, world=world,
                      **keypoint_kw)
    if args.hand_maps:
        from .infer import _rank_world
        from .render import hand_maps_folder
        rank, world = _rank_world(None, None)
        hand_maps_folder(args.input, args.output, args.hand_maps, hamer, k_real, label=args.hand_label, rank=rank, world=world)


if __name__ == '__main__':
    main()
