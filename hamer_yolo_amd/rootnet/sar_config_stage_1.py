"""rootnet/sar_config_stage_1.py:5-23 (the fields the depth path and the SAR head read)."""


class rgb_opt:
    backbone = 'resnet34'
    in_channels = 512
    input_img_shape = (256, 256)
    bbox_real = (0.3, 0.3)
    cam_para = [906.96, 906.79, 1920 // 2, 1080 // 2]
    num_FMs = 8
    feature_size = 64
    heatmap_size = 32
    num_vert = 778
    num_joints = 21
    depth_box = 0.3
    device = 'cuda'
    precise = False                 # True: the fp32 route of the backbone, RootNet and the SAR head (d_infer --precise-rootnet)
    checkpoint = 'synthetic:0'      # the reference hard-codes /home/pt/fbs/model/rootnet/SAR-resnet34-Root.pth
