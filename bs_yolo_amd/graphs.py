"""Stock model descriptions in the reference's yaml-dict schema (what ``model.yaml`` holds on a live reference model).

The reference ships these graphs as cfg/models/11/yolo11-seg.yaml:15-47 (stock YOLO11 backbone+neck),
cfg/models/v8/yolov8-seg.yaml:15-46, cfg/models/v5/yolov5.yaml:14-50, cfg/models/11/yolo11.yaml:15-52 (the modified BS-YOLO
graph, family "bsyolo11") and the four-level variants cfg/models/v8/yolov8-p2.yaml, v8/yolov8-p6.yaml (+ yolov8-seg-p6.yaml) and
v5/yolov5-p6.yaml (families "yolov8-p2", "yolov8-p6", "yolov5-p6"), and the YOLOv9 (GELAN) graphs cfg/models/v9/yolov9{t,s,m,c}.yaml and
yolov9c-seg.yaml (family "yolov9": literal widths per size, no scales table), and the classification graphs
cfg/models/11/yolo11-cls.yaml:8-30 and v8/yolov8-cls.yaml:8-29 (task "classify" of the families "yolo11" and "yolov8"), and the pose
graphs cfg/models/11/yolo11-pose.yaml, v8/yolov8-pose.yaml and v8/yolov8-pose-p6.yaml: the detect graphs of "yolo11", "yolov8" and
"yolov8-p6" under a Pose head, with a top-level `kpt_shape` (task "pose"), and the ghost graphs cfg/models/v8/yolov8-ghost.yaml,
yolov8-ghost-p2.yaml and yolov8-ghost-p6.yaml (families "yolov8-ghost", "yolov8-ghost-p2", "yolov8-ghost-p6": GhostConv downsamplers and
C3Ghost blocks on the YOLOv8 layouts, detect only), and the YOLOv10 graphs cfg/models/v10/yolov10{n,s,m,b,l,x}.yaml (family
"yolov10": one layout, a literal table per size of where C2fCIB stands and whether it holds the 7x7 RepVGGDW; a v10Detect head), and the
YOLOv3 graphs cfg/models/v3/yolov3.yaml, yolov3-spp.yaml and yolov3-tiny.yaml (families "yolov3", "yolov3-spp", "yolov3-tiny": one size
each, `depth_multiple` / `width_multiple` of 1.0 instead of a scales table; detect only), and the open-vocabulary graph
cfg/models/v8/yolov8-worldv2.yaml (family "yolov8-worldv2": C2fAttn neck blocks, a WorldDetect head; detect only), and YOLOv9e,
cfg/models/v9/yolov9e.yaml and yolov9e-seg.yaml (family "yolov9e": one size, two GELAN backbones joined by CBLinear / CBFuse).  They are
restated here as data so the engine can be built where the reference is not installed (benchmarks, GPU box).
"""
from __future__ import annotations

import copy

_UP = [-1, 1, "nn.Upsample", [None, 2, "nearest"]]


def _cat(j):
    return [[-1, j], 1, "Concat", [1]]


_YOLO11 = {
    "scales": {"n": [0.50, 0.25, 1024], "s": [0.50, 0.50, 1024], "m": [0.50, 1.00, 512], "l": [1.00, 1.00, 512],
               "x": [1.00, 1.50, 512]},
    "backbone": [
        [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 2, "C3k2", [256, False, 0.25]],
        [-1, 1, "Conv", [256, 3, 2]], [-1, 2, "C3k2", [512, False, 0.25]], [-1, 1, "Conv", [512, 3, 2]],
        [-1, 2, "C3k2", [512, True]], [-1, 1, "Conv", [1024, 3, 2]], [-1, 2, "C3k2", [1024, True]],
        [-1, 1, "SPPF", [1024, 5]], [-1, 2, "C2PSA", [1024]],
    ],
    "head": [
        _UP, _cat(6), [-1, 2, "C3k2", [512, False]],
        _UP, _cat(4), [-1, 2, "C3k2", [256, False]],
        [-1, 1, "Conv", [256, 3, 2]], _cat(13), [-1, 2, "C3k2", [512, False]],
        [-1, 1, "Conv", [512, 3, 2]], _cat(10), [-1, 2, "C3k2", [1024, True]],
    ],
    "detect_from": [16, 19, 22],
}

_YOLOV8 = {
    "scales": {"n": [0.33, 0.25, 1024], "s": [0.33, 0.50, 1024], "m": [0.67, 0.75, 768], "l": [1.00, 1.00, 512],
               "x": [1.00, 1.25, 512]},
    "backbone": [
        [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 3, "C2f", [128, True]],
        [-1, 1, "Conv", [256, 3, 2]], [-1, 6, "C2f", [256, True]], [-1, 1, "Conv", [512, 3, 2]],
        [-1, 6, "C2f", [512, True]], [-1, 1, "Conv", [1024, 3, 2]], [-1, 3, "C2f", [1024, True]],
        [-1, 1, "SPPF", [1024, 5]],
    ],
    "head": [
        _UP, _cat(6), [-1, 3, "C2f", [512]],
        _UP, _cat(4), [-1, 3, "C2f", [256]],
        [-1, 1, "Conv", [256, 3, 2]], _cat(12), [-1, 3, "C2f", [512]],
        [-1, 1, "Conv", [512, 3, 2]], _cat(9), [-1, 3, "C2f", [1024]],
    ],
    "detect_from": [15, 18, 21],
}

# YOLO-World v2, cfg/models/v8/yolov8-worldv2.yaml:15-46: the YOLOv8 backbone and PAN neck with C2fAttn [c2, ec, nh] (a C2f without shortcuts
# plus a max-sigmoid attention chunk guided by the text features) for the four neck blocks, and the head WorldDetect [nc, embed, with_bn].
# Layer 16 names its input (15), which is the layer before it.  Detect only; v1 (yolov8-world.yaml, ImagePoolingAttn) is not restated
_YOLOV8_WORLDV2 = {
    "scales": _YOLOV8["scales"],
    "backbone": _YOLOV8["backbone"],
    "head": [
        _UP, _cat(6), [-1, 3, "C2fAttn", [512, 256, 8]],
        _UP, _cat(4), [-1, 3, "C2fAttn", [256, 128, 4]],
        [15, 1, "Conv", [256, 3, 2]], _cat(12), [-1, 3, "C2fAttn", [512, 256, 8]],
        [-1, 1, "Conv", [512, 3, 2]], _cat(9), [-1, 3, "C2fAttn", [1024, 512, 16]],
    ],
    "detect_from": [15, 18, 21],
}

# The fork's own graph, cfg/models/11/yolo11.yaml:15-52 (nc = 12 there): C3k2_gai / SCDown / MSCAAttention in the backbone,
# an ELA gate after every neck C3k2, Detect on the ELA outputs.  Layer 21 concatenates layer 13, itself a Concat.
_BSYOLO11 = {
    "scales": _YOLO11["scales"],
    "backbone": [
        [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 2, "C3k2_gai", [256, False, 0.25]],
        [-1, 1, "Conv", [256, 3, 2]], [-1, 2, "C3k2_gai", [512, False, 0.25]], [-1, 1, "SCDown", [512, 3, 2]],
        [-1, 2, "C3k2_gai", [512, True]], [-1, 1, "SCDown", [1024, 3, 2]], [-1, 2, "C3k2_gai", [1024, True]],
        [-1, 1, "SPPF", [1024, 5]], [-1, 2, "C2PSA", [1024]], [-1, 1, "MSCAAttention", []],
    ],
    "head": [
        _UP, _cat(6), [-1, 2, "C3k2", [512, False]], [-1, 1, "ELA", [512]],
        _UP, _cat(4), [-1, 2, "C3k2", [256, False]], [-1, 1, "ELA", [256]],
        [-1, 1, "Conv", [256, 3, 2]], _cat(13), [-1, 2, "C3k2", [512, False]], [-1, 1, "ELA", [512]],
        [-1, 1, "SCDown", [512, 3, 2]], _cat(10), [-1, 2, "C3k2", [1024, True]], [-1, 1, "ELA", [1024]],
    ],
    "detect_from": [19, 23, 27],
}

# YOLOv5u, cfg/models/v5/yolov5.yaml:14-50: 6x6 stride-2 pad-2 stem, C3 blocks, SPPF, the anchor-free Detect head
_YOLOV5 = {
    "scales": {"n": [0.33, 0.25, 1024], "s": [0.33, 0.50, 1024], "m": [0.67, 0.75, 1024], "l": [1.00, 1.00, 1024],
               "x": [1.33, 1.25, 1024]},
    "backbone": [
        [-1, 1, "Conv", [64, 6, 2, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 3, "C3", [128]],
        [-1, 1, "Conv", [256, 3, 2]], [-1, 6, "C3", [256]], [-1, 1, "Conv", [512, 3, 2]],
        [-1, 9, "C3", [512]], [-1, 1, "Conv", [1024, 3, 2]], [-1, 3, "C3", [1024]],
        [-1, 1, "SPPF", [1024, 5]],
    ],
    "head": [
        [-1, 1, "Conv", [512, 1, 1]], _UP, _cat(6), [-1, 3, "C3", [512, False]],
        [-1, 1, "Conv", [256, 1, 1]], _UP, _cat(4), [-1, 3, "C3", [256, False]],
        [-1, 1, "Conv", [256, 3, 2]], _cat(14), [-1, 3, "C3", [512, False]],
        [-1, 1, "Conv", [512, 3, 2]], _cat(10), [-1, 3, "C3", [1024, False]],
    ],
    "detect_from": [17, 20, 23],
}

# Four-level heads.  cfg/models/v8/yolov8-p2.yaml:14-45: the YOLOv8 backbone, a neck that goes one step further up to stride 4,
# Detect on (P2, P3, P4, P5)
_YOLOV8_P2 = {
    "scales": _YOLOV8["scales"],
    "backbone": _YOLOV8["backbone"],
    "head": [
        _UP, _cat(6), [-1, 3, "C2f", [512]],
        _UP, _cat(4), [-1, 3, "C2f", [256]],
        _UP, _cat(2), [-1, 3, "C2f", [128]],
        [-1, 1, "Conv", [128, 3, 2]], _cat(15), [-1, 3, "C2f", [256]],
        [-1, 1, "Conv", [256, 3, 2]], _cat(12), [-1, 3, "C2f", [512]],
        [-1, 1, "Conv", [512, 3, 2]], _cat(9), [-1, 3, "C2f", [1024]],
    ],
    "detect_from": [18, 21, 24, 27],
}

# cfg/models/v8/yolov8-p6.yaml:14-47 (and yolov8-seg-p6.yaml, the same graph under a Segment head): a 768-channel stride-32 stage, a
# stride-64 stage before SPPF, C2 blocks (not C2f) in the neck, the head on (P3, P4, P5, P6)
_YOLOV8_P6 = {
    "scales": _YOLOV8["scales"],
    "backbone": [
        [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 3, "C2f", [128, True]],
        [-1, 1, "Conv", [256, 3, 2]], [-1, 6, "C2f", [256, True]], [-1, 1, "Conv", [512, 3, 2]],
        [-1, 6, "C2f", [512, True]], [-1, 1, "Conv", [768, 3, 2]], [-1, 3, "C2f", [768, True]],
        [-1, 1, "Conv", [1024, 3, 2]], [-1, 3, "C2f", [1024, True]], [-1, 1, "SPPF", [1024, 5]],
    ],
    "head": [
        _UP, _cat(8), [-1, 3, "C2", [768, False]],
        _UP, _cat(6), [-1, 3, "C2", [512, False]],
        _UP, _cat(4), [-1, 3, "C2", [256, False]],
        [-1, 1, "Conv", [256, 3, 2]], _cat(17), [-1, 3, "C2", [512, False]],
        [-1, 1, "Conv", [512, 3, 2]], _cat(14), [-1, 3, "C2", [768, False]],
        [-1, 1, "Conv", [768, 3, 2]], _cat(11), [-1, 3, "C2", [1024, False]],
    ],
    "detect_from": [20, 23, 26, 29],
}

# cfg/models/v5/yolov5-p6.yaml:14-53: YOLOv5u with the same two extra stages, a 1x1 Conv before every upsample
_YOLOV5_P6 = {
    "scales": _YOLOV5["scales"],
    "backbone": [
        [-1, 1, "Conv", [64, 6, 2, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 3, "C3", [128]],
        [-1, 1, "Conv", [256, 3, 2]], [-1, 6, "C3", [256]], [-1, 1, "Conv", [512, 3, 2]],
        [-1, 9, "C3", [512]], [-1, 1, "Conv", [768, 3, 2]], [-1, 3, "C3", [768]],
        [-1, 1, "Conv", [1024, 3, 2]], [-1, 3, "C3", [1024]], [-1, 1, "SPPF", [1024, 5]],
    ],
    "head": [
        [-1, 1, "Conv", [768, 1, 1]], _UP, _cat(8), [-1, 3, "C3", [768, False]],
        [-1, 1, "Conv", [512, 1, 1]], _UP, _cat(6), [-1, 3, "C3", [512, False]],
        [-1, 1, "Conv", [256, 1, 1]], _UP, _cat(4), [-1, 3, "C3", [256, False]],
        [-1, 1, "Conv", [256, 3, 2]], _cat(20), [-1, 3, "C3", [512, False]],
        [-1, 1, "Conv", [512, 3, 2]], _cat(16), [-1, 3, "C3", [768, False]],
        [-1, 1, "Conv", [768, 3, 2]], _cat(12), [-1, 3, "C3", [1024, False]],
    ],
    "detect_from": [23, 26, 29, 32],
}

# YOLOv8-ghost, cfg/models/v8/yolov8-ghost.yaml:15-47: the YOLOv8 layout with a GhostConv for every stride-2 Conv behind the stem and a C3Ghost
# for every C2f; the scales table is YOLOv8's
_YOLOV8_GHOST = {
    "scales": _YOLOV8["scales"],
    "backbone": [
        [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "GhostConv", [128, 3, 2]], [-1, 3, "C3Ghost", [128, True]],
        [-1, 1, "GhostConv", [256, 3, 2]], [-1, 6, "C3Ghost", [256, True]], [-1, 1, "GhostConv", [512, 3, 2]],
        [-1, 6, "C3Ghost", [512, True]], [-1, 1, "GhostConv", [1024, 3, 2]], [-1, 3, "C3Ghost", [1024, True]],
        [-1, 1, "SPPF", [1024, 5]],
    ],
    "head": [
        _UP, _cat(6), [-1, 3, "C3Ghost", [512]],
        _UP, _cat(4), [-1, 3, "C3Ghost", [256]],
        [-1, 1, "GhostConv", [256, 3, 2]], _cat(12), [-1, 3, "C3Ghost", [512]],
        [-1, 1, "GhostConv", [512, 3, 2]], _cat(9), [-1, 3, "C3Ghost", [1024]],
    ],
    "detect_from": [15, 18, 21],
}

# cfg/models/v8/yolov8-ghost-p2.yaml:14-54: the same backbone, the neck one step further up to stride 4, Detect on (P2, P3, P4, P5)
_YOLOV8_GHOST_P2 = {
    "scales": _YOLOV8["scales"],
    "backbone": _YOLOV8_GHOST["backbone"],
    "head": [
        _UP, _cat(6), [-1, 3, "C3Ghost", [512]],
        _UP, _cat(4), [-1, 3, "C3Ghost", [256]],
        _UP, _cat(2), [-1, 3, "C3Ghost", [128]],
        [-1, 1, "GhostConv", [128, 3, 2]], _cat(15), [-1, 3, "C3Ghost", [256]],
        [-1, 1, "GhostConv", [256, 3, 2]], _cat(12), [-1, 3, "C3Ghost", [512]],
        [-1, 1, "GhostConv", [512, 3, 2]], _cat(9), [-1, 3, "C3Ghost", [1024]],
    ],
    "detect_from": [18, 21, 24, 27],
}

# cfg/models/v8/yolov8-ghost-p6.yaml:14-56: a 768-channel stride-32 stage and a stride-64 stage before SPPF, the head on (P3, P4, P5, P6)
_YOLOV8_GHOST_P6 = {
    "scales": _YOLOV8["scales"],
    "backbone": [
        [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "GhostConv", [128, 3, 2]], [-1, 3, "C3Ghost", [128, True]],
        [-1, 1, "GhostConv", [256, 3, 2]], [-1, 6, "C3Ghost", [256, True]], [-1, 1, "GhostConv", [512, 3, 2]],
        [-1, 6, "C3Ghost", [512, True]], [-1, 1, "GhostConv", [768, 3, 2]], [-1, 3, "C3Ghost", [768, True]],
        [-1, 1, "GhostConv", [1024, 3, 2]], [-1, 3, "C3Ghost", [1024, True]], [-1, 1, "SPPF", [1024, 5]],
    ],
    "head": [
        _UP, _cat(8), [-1, 3, "C3Ghost", [768]],
        _UP, _cat(6), [-1, 3, "C3Ghost", [512]],
        _UP, _cat(4), [-1, 3, "C3Ghost", [256]],
        [-1, 1, "GhostConv", [256, 3, 2]], _cat(17), [-1, 3, "C3Ghost", [512]],
        [-1, 1, "GhostConv", [512, 3, 2]], _cat(14), [-1, 3, "C3Ghost", [768]],
        [-1, 1, "GhostConv", [768, 3, 2]], _cat(11), [-1, 3, "C3Ghost", [1024]],
    ],
    "detect_from": [20, 23, 26, 29],
}


# YOLOv9 (GELAN), cfg/models/v9/yolov9{t,s,m,c}.yaml:7-41: one layout for all four sizes -- stem, four ELAN stages with a
# downsampling block in front of each, SPPELAN, a PAN neck of four more ELAN blocks -- and no `scales:` table: every size is its own
# file with literal widths.  Per size: the two stem widths; the block of layer 2 (t / s: ELAN1, m / c: RepNCSPELAN4) with its
# arguments; the downsampling block (t / s / m: AConv, c: ADown); [c2, c3, c4] of the P3 / P4 / P5 stages (the neck reuses them);
# RepCSP's repeat count; SPPELAN's [c2, c3]; the widths of the two downsampling blocks of the neck.
_V9_SIZES = {
    "t": dict(stem=(16, 32), l2=("ELAN1", [32, 32, 16]), down="AConv", stages=([64, 64, 32], [96, 96, 48], [128, 128, 64]), n=3,
              spp=[128, 64], neck_down=(48, 64)),
    "s": dict(stem=(32, 64), l2=("ELAN1", [64, 64, 32]), down="AConv", stages=([128, 128, 64], [192, 192, 96], [256, 256, 128]), n=3,
              spp=[256, 128], neck_down=(96, 128)),
    "m": dict(stem=(32, 64), l2=("RepNCSPELAN4", [128, 128, 64, 1]), down="AConv",
              stages=([240, 240, 120], [360, 360, 180], [480, 480, 240]), n=1, spp=[480, 240], neck_down=(180, 240)),
    "c": dict(stem=(64, 128), l2=("RepNCSPELAN4", [256, 128, 64, 1]), down="ADown",
              stages=([512, 256, 128], [512, 512, 256], [512, 512, 256]), n=1, spp=[512, 256], neck_down=(256, 512)),
}


def _yolov9(size: str) -> dict:
    z = _V9_SIZES[size]
    p3, p4, p5 = ([-1, 1, "RepNCSPELAN4", a + [z["n"]]] for a in z["stages"])
    down = lambda c: [-1, 1, z["down"], [c]]
    n3 = list(p3)
    if size == "c":  # yolov9c.yaml:29: the neck's P3 block is [256, 256, 128, 1], the backbone's [512, 256, 128, 1]
        n3 = [-1, 1, "RepNCSPELAN4", [256, 256, 128, 1]]
    return {
        "backbone": [
            [-1, 1, "Conv", [z["stem"][0], 3, 2]], [-1, 1, "Conv", [z["stem"][1], 3, 2]], [-1, 1, z["l2"][0], list(z["l2"][1])],
            down(z["stages"][0][0] if size != "c" else 256), p3, down(z["stages"][1][0]), p4, down(z["stages"][2][0]), p5,
            [-1, 1, "SPPELAN", list(z["spp"])],
        ],
        "head": [
            _UP, _cat(6), list(p4),
            _UP, _cat(4), n3,
            down(z["neck_down"][0]), _cat(12), list(p4),
            down(z["neck_down"][1]), _cat(9), list(p5),
        ],
        "detect_from": [15, 18, 21],
    }


# YOLOv9e, cfg/models/v9/yolov9e.yaml:9-63 (yolov9e-seg.yaml: the same graph under Segment): an nn.Identity that names the image, a first
# GELAN backbone (layers 1-9) whose five maps each feed a CBLinear (10-14: a biased 1x1 conv split into one group per stage up to its
# own), and a second backbone (15-28) of the same stem / ADown / RepNCSPELAN4 steps that starts from the image again and adds, after each
# step, group s of every CBLinear at stage s or deeper (CBFuse, nearest-upsampled); then SPPELAN and yolov9c's neck layout.  One size,
# literal widths: the two stem widths, [c2, c3, c4] of the four stages (RepCSP repeats n), SPPELAN's [c2, c3], the neck's four blocks.
_V9E = dict(stem=(64, 128), stages=([256, 128, 64], [512, 256, 128], [1024, 512, 256], [1024, 512, 256]), n=2, spp=[512, 256],
            neck=([512, 512, 256], [256, 256, 128], [512, 512, 256], [512, 1024, 512]))


def _yolov9e() -> dict:
    z = _V9E
    elan = lambda a: [-1, 1, "RepNCSPELAN4", list(a) + [z["n"]]]
    down = lambda c: [-1, 1, "ADown", [c]]
    s = [elan(a) for a in z["stages"]]
    groups = [z["stem"][0], z["stem"][1]] + [a[0] for a in z["stages"][:3]]  # the width of each step's map: what a CBFuse there adds
    first = [[-1, 1, "Conv", [z["stem"][0], 3, 2]], [-1, 1, "Conv", [z["stem"][1], 3, 2]], s[0], down(groups[2]), s[1], down(groups[3]), s[2],
             down(groups[4]), s[3]]  # layers 1-9
    taps = [[src, 1, "CBLinear", [groups[:j + 1]]] for j, src in enumerate((1, 3, 5, 7, 9))]  # layers 10-14
    fuse = lambda j: [list(range(10 + j, 15)) + [-1], 1, "CBFuse", [[j] * (5 - j)]]
    second = [[0, 1, "Conv", [z["stem"][0], 3, 2]], fuse(0), [-1, 1, "Conv", [z["stem"][1], 3, 2]], fuse(1), elan(z["stages"][0]), down(groups[2]),
              fuse(2), elan(z["stages"][1]), down(groups[3]), fuse(3), elan(z["stages"][2]), down(groups[4]), fuse(4), elan(z["stages"][3])]  # 15-28
    n = [elan(a) for a in z["neck"]]
    return {
        "backbone": [[-1, 1, "nn.Identity", []]] + first + taps + second + [[-1, 1, "SPPELAN", list(z["spp"])]],
        "head": [_UP, _cat(25), n[0], _UP, _cat(22), n[1], down(n[1][3][0]), _cat(32), n[2], down(n[2][3][0]), _cat(29), n[3]],
        "detect_from": [35, 38, 41],
    }


# YOLOv10, cfg/models/v10/yolov10{n,s,m,b,l,x}.yaml:6-41: the YOLOv8 layout with SCDown for the stride-2 convs of P4 / P5 (and of the neck's
# last step), PSA behind SPPF and the NMS-free v10Detect head.  Every size is its own file with a one-entry `scales` table; they differ in
# which of layers 6, 8, 13, 19, 22 are C2fCIB instead of C2f and in C2fCIB's `lk` argument (RepVGGDW 7x7; n and s only).
_V10_SIZES = {
    "n": dict(scale=[0.33, 0.25, 1024], cib=(22,), lk=True),
    "s": dict(scale=[0.33, 0.50, 1024], cib=(8, 22), lk=True),
    "m": dict(scale=[0.67, 0.75, 768], cib=(8, 19, 22), lk=False),
    "b": dict(scale=[0.67, 1.00, 512], cib=(8, 13, 19, 22), lk=False),
    "l": dict(scale=[1.00, 1.00, 512], cib=(8, 13, 19, 22), lk=False),
    "x": dict(scale=[1.00, 1.25, 512], cib=(6, 8, 13, 19, 22), lk=False),
}


def _yolov10(size: str) -> dict:
    z = _V10_SIZES[size]

    def blk(i, n, c2, backbone):
        if i in z["cib"]:
            return [-1, n, "C2fCIB", [c2, True, True] if z["lk"] else [c2, True]]
        return [-1, n, "C2f", [c2, True] if backbone else [c2]]

    return {
        "scales": {size: list(z["scale"])},
        "backbone": [
            [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Conv", [128, 3, 2]], blk(2, 3, 128, True),
            [-1, 1, "Conv", [256, 3, 2]], blk(4, 6, 256, True), [-1, 1, "SCDown", [512, 3, 2]],
            blk(6, 6, 512, True), [-1, 1, "SCDown", [1024, 3, 2]], blk(8, 3, 1024, True),
            [-1, 1, "SPPF", [1024, 5]], [-1, 1, "PSA", [1024]],
        ],
        "head": [
            _UP, _cat(6), blk(13, 3, 512, False),
            _UP, _cat(4), blk(16, 3, 256, False),
            [-1, 1, "Conv", [256, 3, 2]], _cat(13), blk(19, 3, 512, False),
            [-1, 1, "SCDown", [512, 3, 2]], _cat(10), blk(22, 3, 1024, False),
        ],
        "detect_from": [16, 19, 22],
    }


# YOLOv3, cfg/models/v3/yolov3.yaml:10-46: darknet-53 -- a stride-1 image conv, then top-level Bottlenecks (chains of up to 8, parse_model's
# nn.Sequential) between stride-2 convs -- and a head of Bottlenecks without shortcut, the first of each upper level reading the Concat
# of an upsampled map directly (a 3x3 conv over it).  yolov3-spp.yaml differs in layer 12 alone: SPP instead of a 1x1 Conv.
def _yolov3(spp: bool) -> dict:
    return {
        "backbone": [
            [-1, 1, "Conv", [32, 3, 1]], [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Bottleneck", [64]],
            [-1, 1, "Conv", [128, 3, 2]], [-1, 2, "Bottleneck", [128]], [-1, 1, "Conv", [256, 3, 2]],
            [-1, 8, "Bottleneck", [256]], [-1, 1, "Conv", [512, 3, 2]], [-1, 8, "Bottleneck", [512]],
            [-1, 1, "Conv", [1024, 3, 2]], [-1, 4, "Bottleneck", [1024]],
        ],
        "head": [
            [-1, 1, "Bottleneck", [1024, False]], [-1, 1, "SPP", [512, [5, 9, 13]]] if spp else [-1, 1, "Conv", [512, 1, 1]],
            [-1, 1, "Conv", [1024, 3, 1]], [-1, 1, "Conv", [512, 1, 1]], [-1, 1, "Conv", [1024, 3, 1]],
            [-2, 1, "Conv", [256, 1, 1]], _UP, _cat(8),
            [-1, 1, "Bottleneck", [512, False]], [-1, 1, "Bottleneck", [512, False]], [-1, 1, "Conv", [256, 1, 1]], [-1, 1, "Conv", [512, 3, 1]],
            [-2, 1, "Conv", [128, 1, 1]], _UP, _cat(6),
            [-1, 1, "Bottleneck", [256, False]], [-1, 2, "Bottleneck", [256, False]],
        ],
        "detect_from": [27, 22, 15],
    }


# cfg/models/v3/yolov3-tiny.yaml:10-37: conv / max-pool pairs down to stride 32, a zero pad + stride-1 pool that keeps the 1/32 map's size, and
# a two-level head (P4, P5) whose upper level is one 3x3 conv over the Concat of an upsampled map
_YOLOV3_TINY = {
    "backbone": [
        [-1, 1, "Conv", [16, 3, 1]], [-1, 1, "nn.MaxPool2d", [2, 2, 0]], [-1, 1, "Conv", [32, 3, 1]], [-1, 1, "nn.MaxPool2d", [2, 2, 0]],
        [-1, 1, "Conv", [64, 3, 1]], [-1, 1, "nn.MaxPool2d", [2, 2, 0]], [-1, 1, "Conv", [128, 3, 1]], [-1, 1, "nn.MaxPool2d", [2, 2, 0]],
        [-1, 1, "Conv", [256, 3, 1]], [-1, 1, "nn.MaxPool2d", [2, 2, 0]], [-1, 1, "Conv", [512, 3, 1]],
        [-1, 1, "nn.ZeroPad2d", [[0, 1, 0, 1]]], [-1, 1, "nn.MaxPool2d", [2, 1, 0]],
    ],
    "head": [
        [-1, 1, "Conv", [1024, 3, 1]], [-1, 1, "Conv", [256, 1, 1]], [-1, 1, "Conv", [512, 3, 1]],
        [-2, 1, "Conv", [128, 1, 1]], _UP, _cat(8), [-1, 1, "Conv", [256, 3, 1]],
    ],
    "detect_from": [19, 15],
}
_V3_FAMILIES = {"yolov3": lambda: _yolov3(False), "yolov3-spp": lambda: _yolov3(True), "yolov3-tiny": lambda: _YOLOV3_TINY}


# YOLOv6-3.0, cfg/models/v6/yolov6.yaml:5-53: 3x3 / 1x1 Convs only -- stride-2 convs with chains of equal-width 3x3 Convs behind them
# (repeats 6 / 12 / 18 / 6 in the backbone, 9 in every neck stage; parse_model's nn.Sequential) --, one SPPF, two nn.ConvTranspose2d
# upsamplers and a legacy Detect; `activation: nn.ReLU()` at the top (plan.py Plan.sppf_act on what that means for SPPF)
_YOLOV6 = {
    "scales": {"n": [0.33, 0.25, 1024], "s": [0.33, 0.50, 1024], "m": [0.67, 0.75, 768], "l": [1.00, 1.00, 512], "x": [1.00, 1.25, 512]},
    "backbone": [
        [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 6, "Conv", [128, 3, 1]],
        [-1, 1, "Conv", [256, 3, 2]], [-1, 12, "Conv", [256, 3, 1]], [-1, 1, "Conv", [512, 3, 2]],
        [-1, 18, "Conv", [512, 3, 1]], [-1, 1, "Conv", [1024, 3, 2]], [-1, 6, "Conv", [1024, 3, 1]],
        [-1, 1, "SPPF", [1024, 5]],
    ],
    "head": [
        [-1, 1, "Conv", [256, 1, 1]], [-1, 1, "nn.ConvTranspose2d", [256, 2, 2, 0]], _cat(6), [-1, 1, "Conv", [256, 3, 1]], [-1, 9, "Conv", [256, 3, 1]],
        [-1, 1, "Conv", [128, 1, 1]], [-1, 1, "nn.ConvTranspose2d", [128, 2, 2, 0]], _cat(4), [-1, 1, "Conv", [128, 3, 1]], [-1, 9, "Conv", [128, 3, 1]],
        [-1, 1, "Conv", [128, 3, 2]], _cat(15), [-1, 1, "Conv", [256, 3, 1]], [-1, 9, "Conv", [256, 3, 1]],
        [-1, 1, "Conv", [256, 3, 2]], _cat(10), [-1, 1, "Conv", [512, 3, 1]], [-1, 9, "Conv", [512, 3, 1]],
    ],
    "detect_from": [19, 23, 27],
}


# Classification graphs: backbones and scales tables of their own, one Classify layer as the head.  cfg/models/11/yolo11-cls.yaml:8-30:
# the detect backbone without SPPF, and C2PSA reaches max_channels at m / l / x (512, where detect's table says the same)
_YOLO11_CLS = {
    "scales": {"n": [0.50, 0.25, 1024], "s": [0.50, 0.50, 1024], "m": [0.50, 1.00, 512], "l": [1.00, 1.00, 512],
               "x": [1.00, 1.50, 512]},
    "backbone": [
        [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 2, "C3k2", [256, False, 0.25]],
        [-1, 1, "Conv", [256, 3, 2]], [-1, 2, "C3k2", [512, False, 0.25]], [-1, 1, "Conv", [512, 3, 2]],
        [-1, 2, "C3k2", [512, True]], [-1, 1, "Conv", [1024, 3, 2]], [-1, 2, "C3k2", [1024, True]],
        [-1, 2, "C2PSA", [1024]],
    ],
}

# cfg/models/v8/yolov8-cls.yaml:8-29: no SPPF, and every scale's max_channels is 1024 (detect's m / l / x: 768 / 512 / 512)
_YOLOV8_CLS = {
    "scales": {"n": [0.33, 0.25, 1024], "s": [0.33, 0.50, 1024], "m": [0.67, 0.75, 1024], "l": [1.00, 1.00, 1024],
               "x": [1.00, 1.25, 1024]},
    "backbone": [
        [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 3, "C2f", [128, True]],
        [-1, 1, "Conv", [256, 3, 2]], [-1, 6, "C2f", [256, True]], [-1, 1, "Conv", [512, 3, 2]],
        [-1, 6, "C2f", [512, True]], [-1, 1, "Conv", [1024, 3, 2]], [-1, 3, "C2f", [1024, True]],
    ],
}

_CLS_FAMILIES = {"yolo11": _YOLO11_CLS, "yolov8": _YOLOV8_CLS}
_POSE_FAMILIES = ("yolo11", "yolov8", "yolov8-p6")  # the families the reference ships a -pose yaml for
_FAMILIES = {"yolo11": _YOLO11, "yolov8": _YOLOV8, "bsyolo11": _BSYOLO11, "yolov5": _YOLOV5,
             "yolov8-p2": _YOLOV8_P2, "yolov8-p6": _YOLOV8_P6, "yolov5-p6": _YOLOV5_P6,
             "yolov8-ghost": _YOLOV8_GHOST, "yolov8-ghost-p2": _YOLOV8_GHOST_P2, "yolov8-ghost-p6": _YOLOV8_GHOST_P6}


def stock_cfg(family: str = "yolo11", scale: str = "s", nc: int = 80, task: str = "detect", kpt_shape=None) -> dict:
    """e.g. stock_cfg("yolo11", "s") == what the reference builds for 'yolo11s.yaml' upstream; stock_cfg("yolov9", "c", task="segment")
    == 'yolov9c-seg.yaml' (family "yolov9": scale is one of t / s / m / c, segment exists for c only; the dict has no `scales`);
    stock_cfg("yolo11", "n", 1000, "classify") == 'yolo11n-cls.yaml' (families "yolo11" and "yolov8" only);
    stock_cfg("yolo11", "n", 1, "pose", kpt_shape=(17, 3)) == 'yolo11n-pose.yaml' (families "yolo11", "yolov8" and "yolov8-p6" only;
    `kpt_shape` = (keypoints, 2 or 3 channels each) is read by this task alone, becomes the dict's top-level `kpt_shape` and has to be
    given: the four-argument call stock_cfg(family, scale, nc, "pose") raises ValueError for every family, as it always has);
    stock_cfg("yolov10", "s") == 'yolov10s.yaml' (scales n, s, m, b, l, x; detect only);
    stock_cfg("yolov3-tiny", None) == 'yolov3-tiny.yaml' (families "yolov3", "yolov3-spp", "yolov3-tiny": one size each, so `scale` must be
    None or ""; detect only; the dict carries depth_multiple = width_multiple = 1.0 and no `scales`);
    stock_cfg("yolov8-worldv2", "s") == 'yolov8s-worldv2.yaml' (scales n, s, m, l, x; detect only);
    stock_cfg("yolov9e", None) == 'yolov9e.yaml', with task="segment" 'yolov9e-seg.yaml' (family "yolov9e": one size, `scale` None or "";
    stock_cfg("yolov9", "e") stays a ValueError)."""
    if family in _V3_FAMILIES:
        if scale not in (None, "") or task != "detect":
            raise ValueError(f"{family}: scale {scale!r} / task {task!r} (one size, scale None; detect only)")
        fam = copy.deepcopy(_V3_FAMILIES[family]())
        return {"nc": nc, "depth_multiple": 1.0, "width_multiple": 1.0, "backbone": fam["backbone"],
                "head": fam["head"] + [[fam["detect_from"], 1, "Detect", ["nc"]]]}
    if task == "classify":
        if family not in _CLS_FAMILIES:
            raise ValueError(f"{family}: no classification graph (yolo11, yolov8)")
        fam = copy.deepcopy(_CLS_FAMILIES[family])
        return {"nc": nc, "scale": scale, "scales": fam["scales"], "backbone": fam["backbone"], "head": [[-1, 1, "Classify", ["nc"]]]}
    if task == "pose" and family not in _POSE_FAMILIES:
        raise ValueError(f"{family}: no pose graph ({', '.join(_POSE_FAMILIES)})")
    if task == "pose" and kpt_shape is None:
        raise ValueError("pose: kpt_shape=(keypoints, channels of each) is needed (the reference's yamls say (17, 3))")
    if family == "yolov9e":  # one size: two backbones joined by CBLinear / CBFuse; no `scales`, literal widths like "yolov9"
        if scale not in (None, "") or task not in ("detect", "segment"):
            raise ValueError(f"yolov9e: scale {scale!r} / task {task!r} (one size, scale None; detect and segment)")
        fam = _yolov9e()
        head = fam["head"] + [[fam["detect_from"], 1, "Detect", ["nc"]] if task == "detect" else [fam["detect_from"], 1, "Segment", ["nc", 32, 256]]]
        return {"nc": nc, "backbone": fam["backbone"], "head": head}
    if family == "yolov9":
        if scale not in _V9_SIZES or task not in ("detect", "segment") or (task == "segment" and scale != "c"):
            raise ValueError(f"yolov9: scale {scale!r} / task {task!r} (detect: t, s, m, c; segment: c)")
        fam = copy.deepcopy(_yolov9(scale))
        head = fam["head"] + [[fam["detect_from"], 1, "Detect", ["nc"]] if task == "detect" else [fam["detect_from"], 1, "Segment", ["nc", 32, 256]]]
        return {"nc": nc, "backbone": fam["backbone"], "head": head}
    if family == "yolov10":  # detect only, under the v10Detect head; `scales` holds the one entry its yaml has
        if scale not in _V10_SIZES or task != "detect":
            raise ValueError(f"yolov10: scale {scale!r} / task {task!r} (detect: n, s, m, b, l, x)")
        fam = copy.deepcopy(_yolov10(scale))
        return {"nc": nc, "scale": scale, "scales": fam["scales"], "backbone": fam["backbone"],
                "head": fam["head"] + [[fam["detect_from"], 1, "v10Detect", ["nc"]]]}
    if family == "yolov6":  # detect only; the one stock graph with an `activation` key
        if scale not in _YOLOV6["scales"] or task != "detect":
            raise ValueError(f"yolov6: scale {scale!r} / task {task!r} (detect: n, s, m, l, x)")
        fam = copy.deepcopy(_YOLOV6)
        return {"nc": nc, "activation": "nn.ReLU()", "scale": scale, "scales": fam["scales"], "backbone": fam["backbone"],
                "head": fam["head"] + [[fam["detect_from"], 1, "Detect", ["nc"]]]}
    if family == "yolov8-worldv2":  # detect only, under WorldDetect [nc, 512, True] (the BatchNorm contrastive head)
        if scale not in _YOLOV8_WORLDV2["scales"] or task != "detect":
            raise ValueError(f"yolov8-worldv2: scale {scale!r} / task {task!r} (detect: n, s, m, l, x)")
        fam = copy.deepcopy(_YOLOV8_WORLDV2)
        return {"nc": nc, "scale": scale, "scales": fam["scales"], "backbone": fam["backbone"],
                "head": fam["head"] + [[fam["detect_from"], 1, "WorldDetect", ["nc", 512, True]]]}
    fam = copy.deepcopy(_FAMILIES[family])
    head = list(fam["head"])
    if task == "detect":
        head.append([fam["detect_from"], 1, "Detect", ["nc"]])
    elif task == "segment":
        head.append([fam["detect_from"], 1, "Segment", ["nc", 32, 256]])
    elif task == "obb":  # cfg/models/11/yolo11-obb.yaml:47, v8/yolov8-obb.yaml:46
        head.append([fam["detect_from"], 1, "OBB", ["nc", 1]])
    elif task == "pose":  # cfg/models/11/yolo11-pose.yaml:48, v8/yolov8-pose.yaml:47, v8/yolov8-pose-p6.yaml:57
        head.append([fam["detect_from"], 1, "Pose", ["nc", "kpt_shape"]])
        return {"nc": nc, "kpt_shape": [int(v) for v in kpt_shape], "scale": scale, "scales": fam["scales"], "backbone": fam["backbone"],
                "head": head}
    else:
        raise ValueError(task)
    return {"nc": nc, "scale": scale, "scales": fam["scales"], "backbone": fam["backbone"], "head": head}
