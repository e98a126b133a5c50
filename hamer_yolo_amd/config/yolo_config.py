"""YOLOv7 detector options (reference: config/yolo_config.py:4-15; same attribute names)."""
import os

from .config import opt


class Config:
    weights = os.environ.get("YOLO_WEIGHTS", os.path.join(opt.root_dir, "checkpoints/yolov7_best.pt"))
    imgsz = 640
    augment = True        # ignored, as in the reference: TracedModel.forward drops it (torch_utils.py:371-374)
    conf_thres = 0.25
    iou_thres = 0.35
    classes = [0, 1, 2]
    agnostic_nms = True
    device = "cuda"
    save_path = "./output"
    precise = False       # True: the fp32 detector route (the reference's CPU branch, detector.py:110-112 half = False)
    tta = False           # True: test-time augmentation, Model.forward(x, augment=True) (yolo.py:589-605): scales 1, 0.83 mirrored
                          # and 0.67, one NMS, ~2.2x the detector time.  NOT `augment` above, which stays ignored as the reference
                          # ignores it -- this is the switch that does what that name promises


yolo_opt = Config()
