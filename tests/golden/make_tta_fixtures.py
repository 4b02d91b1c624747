#!/usr/bin/env python3
"""Generate tests/golden/tta.npz by RUNNING THE REFERENCE's test-time augmentation (build container only).

    python tests/golden/make_tta_fixtures.py

DetectionModel(x, augment=True) -> _predict_augment (nn/tasks.py:354-370) on the CPU in fp32, with the reference imported and its
absent third-party modules stood in exactly as make_fixtures.py does (this script imports it for that, and for build_ref).
  geometry   scale_img's padded and resized sizes per pass (run on a dummy tensor of ones: the resized region stays 1.0, the pad is
             0.447), the anchors each pass's prediction has (the model run at the padded size) and _clip_augmented's kept windows
             (read back from index tensors passed through it), for 640x640, 1280x1280, 640x480, 480x640 and 128x192.
  graphs     YOLO11n (80 classes) at (2, 3, 128, 192) and the fork's BS-YOLO11n (nc = 12) at (1, 3, 160, 224): y's shape and y at
             every STRIDE-th anchor (every pass's window, flipped and not, is sampled); x is not stored -- the test regenerates it from
             its seed (torch.rand on a seeded CPU generator) and checks it against the checksum kept here.
  bus        config1_bus.npz's photograph, letterbox and class-bias shift (make_fixtures.config1_fixture): the TTA y at its 300
             highest-scoring anchors (every NMS candidate -- 171 pass conf 0.25 -- with a margin) and non_max_suppression(y, 0.25,
             0.7) -- torchvision's nms bound to the oracle's greedy_nms.
The file stays small (a few hundred kB): only what the comparisons read is stored.
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_fixtures as MF  # noqa: E402  (stand-ins + the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ultralytics.utils.torch_utils import scale_img  # noqa: E402

GEOM_SHAPES = [(640, 640), (1280, 1280), (640, 480), (480, 640), (128, 192)]
SCALES, FLIPS = [1, 0.83, 0.67], [None, 3, None]  # tasks.py:361-362
STRIDE = {"yolo11n": 4, "bsyolo11n": 2}  # stored anchors of the graph cases
BUS_TOP = 300


def geometry(m):
    gs = int(m.stride.max())
    out = {}
    for h, w in GEOM_SHAPES:
        padded, resized, anchors = [], [], []
        for si in SCALES:
            xi = scale_img(torch.ones(1, 1, h, w), si, gs=gs)
            ph, pw = xi.shape[-2:]
            padded.append([ph, pw])
            resized.append([int((xi[0, 0, :, 0] == 1).sum()), int((xi[0, 0, 0, :] == 1).sum())])
            with torch.inference_mode():
                anchors.append(int(m(torch.zeros(1, 3, ph, pw))[0].shape[-1]))
        idx = m._clip_augmented([torch.arange(a, dtype=torch.float64)[None, None] for a in anchors])
        windows = [[int(t[0, 0, 0]), int(t[0, 0, -1]) + 1] for t in idx]
        out[f"{h}x{w}"] = {"padded": padded, "resized": resized, "anchors": anchors, "windows": windows,
                           "total": sum(e - b for b, e in windows)}
        print("geometry", h, w, out[f"{h}x{w}"])
    return out


def graph_case(tag, family, nc, shape, seed):
    m, _, _ = MF.build_ref(family, "n", "detect", nc, 0)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(seed))
    with torch.inference_mode():
        y, aux = m(x, augment=True)
    assert aux is None
    idx = torch.arange(0, y.shape[-1], STRIDE[tag])
    print(tag, tuple(y.shape), len(idx), "anchors stored")
    return {f"{tag}_y_shape": np.array(y.shape), f"{tag}_y_idx": idx.numpy().astype(np.int32), f"{tag}_y": y[..., idx].numpy()}, \
        {"shape": list(shape), "seed": seed, "x_sum": float(x.double().sum()), "x_first": x.flatten()[:8].tolist()}, m


def bus_case():
    from ultralytics.data.augment import LetterBox
    z = np.load(HERE / "config1_bus.npz")
    meta = json.loads(str(z["meta"]))
    bgr = z["bgr"]
    m, _, _ = MF.build_ref("yolo11", "n", "detect", 80, meta["seed"])
    with torch.no_grad():
        for seq in m.model[-1].cv3:
            seq[-1].bias.add_(meta["cls_shift"])
    lb = LetterBox((640, 640), auto=True, stride=32)(image=bgr)
    assert list(lb.shape) == meta["lb_shape"]
    x = torch.from_numpy(np.ascontiguousarray(lb[None][..., ::-1].transpose(0, 3, 1, 2))).float() / 255.0
    with torch.inference_mode():
        y, _ = m(x, augment=True)
        pred = MF.rops.non_max_suppression(y.clone(), meta["conf"], meta["iou"], max_det=300)[0]
    idx = torch.argsort(y[0, 4:].amax(0), descending=True)[:BUS_TOP].sort().values
    print("bus", tuple(y.shape), pred.shape[0], "detections")
    return {"bus_y_shape": np.array(y.shape), "bus_y_idx": idx.numpy(), "bus_y_top": y[0][:, idx].numpy(), "bus_pred": pred.numpy()}


if __name__ == "__main__":
    torch.set_num_threads(8)
    out = {}
    a, xa, m = graph_case("yolo11n", "yolo11", 80, (2, 3, 128, 192), 300)
    out.update(a)
    b, xb, _ = graph_case("bsyolo11n", "bsyolo11", 12, (1, 3, 160, 224), 301)
    out.update(b)
    out.update(bus_case())
    out["meta"] = json.dumps({"geometry": geometry(m), "scales": SCALES, "flips": FLIPS,
                              "cases": {"yolo11n": {"family": "yolo11", "scale": "n", "nc": 80, "seed": 0, "x": xa},
                                        "bsyolo11n": {"family": "bsyolo11", "scale": "n", "nc": 12, "seed": 0, "x": xb}}})
    np.savez_compressed(HERE / "tta.npz", **out)
    print("wrote tta.npz", (HERE / "tta.npz").stat().st_size, "bytes")
