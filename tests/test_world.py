"""YOLO-World v2 graphs on the engine (cfg/models/v8/yolov8-worldv2.yaml: C2fAttn neck blocks, a WorldDetect head) and BSY_OP_MAXSIG, the
max-sigmoid gate of C2fAttn's attention chunk (csrc/maxsig.hip).

Host side (anywhere): graphs.stock_cfg("yolov8-worldv2", ...) against the parsed yaml the fixtures carry; the plans of every scale in every
precision -- four MAXSIG ops, each behind the 3x3 proj_conv (act = 0) whose destination it gates in place --; `text_nc` against cfg["nc"]; what
is refused; the two weight records that fold the text features in ("maxsig", "world_cls") against the modules' formulas in float64; the
reference's parameter names.

MAXSIG alone (``pytest -m gpu``): one-op plans on poisoned views (NaN around the sources, 777 around the destination, NaN between the blob's
records), both storage types, maps of 15 and 189 pixels per image at B = 2 (below one 32-pixel block; a partial last block),
(heads, hc) in (1, 32), (3, 32), (2, 64), (4, 16), nc in 1, 12, 31, 32, 33, 100 (and 1203 on the larger map), in place and out of place.
Bounds (U = 2^-24; ref = the float64 value proj * scale * sigmoid(max_n <e, G_n> + bias)):
  (a), (b) dyadic payloads -- embedding in eighths, |e| <= 2, guide in {-1, -1/2, 0, 1/2, 1}, bias in eighths: every product is a multiple of
      1/16 and every partial sum stays below 2^10 (asserted), so t is exact in f32 in ANY summation order.
      fp16 storage: |got - ref| <= 1 f16 ulp of ref (correct rounding gives 1/2; the f32 sigmoid's few-ulp error can move a value across one
      rounding boundary and no further).
      fp32 storage: |got - ref| <= 8 U |ref| (+ the f32 subnormal spacing): expf <= 2 ulp, carried into 1 / (1 + e) with a factor e / (1 + e) < 1;
      the add 1/2, the division <= 2.5, the two products 1/2 each: 6 ulp, bound 8.
  (c) random payloads: the dot products carry f32 summation error.  |max_n a_n - max_n b_n| <= max_n |a_n - b_n|, a length-hc f32 sum priced as
      op_plan_helpers._bound prices a conv with K = hc: dt = 1.1 hc U max_n sum_k |e_k G_nk| + U |t| (the bias add); sigmoid's slope is at most
      1/4: |got - ref| <= |proj scale| dt / 4 + 8 U |ref| + rounding (half an f16 ulp of ref / U |ref|).

Graphs (``pytest -m gpu``): the three fixtures of tests/golden/make_world_fixtures.py x fp16 / fp32x / fp32 x both shapes against the stored y, raw
maps and NMS rows, and scale n under the 5-row text.  Bounds, the project's own (tests/test_p2p6.py as tests/test_ghost.py states them): fp16
score < 1e-2, box < max(1, stride / 32) px per level, raw maps 3e-2 of max(1, maximum); fp32 / fp32x 1e-3 and 1e-3 * imgsz (raw maps 1e-3 of
max(1, maximum)).  The reference's own fp16 run is within half of the fp16 bounds (meta["ref_fp16"], checked by the generator).
"""
import ctypes as C
import copy
import math
import re
from functools import lru_cache

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from bs_yolo_amd import lib as L
from bs_yolo_amd.graphs import stock_cfg
from bs_yolo_amd.plan import Plan, WRec
from bs_yolo_amd import weights as Wt
from graph_helpers import RawBounds, RefModel, YBounds, cfg_of, check_raw, check_y, fixture, kinds, level_of_anchor, outputs, state_dict, x_of
from op_plan_helpers import DEV, NAN, POISON16, POISON32, U, assert_outside_views_intact, bits, new_op, poisoned, poisoned_blob, run_ops, ulp16, ulp32, view

gpu = pytest.mark.gpu
ROOT = GOLDEN.parent.parent
NC, NC2, E = 12, 5, 512
F16, F32, F64 = torch.float16, torch.float32, torch.float64
GRAPHS = ["yolov8n_worldv2", "yolov8s_worldv2", "yolov8m_worldv2"]
SCALES = ["n", "s", "m", "l", "x"]
PRECISIONS = ["fp16", "fp32x", "fp32"]
ATTN = (12, 15, 18, 21)
HEADS = {"n": [2, 1, 2, 4], "s": [4, 2, 4, 8], "m": [6, 3, 6, 9]}
# fp16: score < 1e-2, box < max(1, stride / 32) px per level, raw maps 3e-2 of max(1, maximum); fp32 / fp32x: 1e-3 and 1e-3 * imgsz
Y_BOUNDS = YBounds(score16=1e-2, p999_16=None, box16=1.0, score32=1e-3, box32=1e-3)
RAW_BOUNDS = RawBounds(rel16=3e-2, strict16=False, floor16=True, rel32=1e-3)


@lru_cache(maxsize=None)
def _texts():
    """The two text sets of make_world_fixtures.py: 12 unit rows from seed 7, 5 from seed 8."""
    t1 = torch.nn.functional.normalize(torch.randn(1, NC, E, generator=torch.Generator().manual_seed(7)), dim=-1)
    t2 = torch.nn.functional.normalize(torch.randn(1, NC2, E, generator=torch.Generator().manual_seed(8)), dim=-1)
    for t, want in zip((t1, t2), fixture(GRAPHS[0])[1]["txt"]):
        assert abs(float(t.double().sum()) - want["sum"]) < 1e-9 * t.numel() and t.flatten()[:8].tolist() == want["first"]
    return t1, t2


def _hit(name, rule):  # make_world_fixtures.py's `hit`
    return rule["contains"] in name and name.endswith(rule["suffix"]) and not name.endswith("norm.bias")


def _damp(name, meta):
    """The factor the generator wrote into meta["damp"] for this name (its rules apply in turn; no two hit the same name)."""
    factors = [rule["factor"] for rule in meta["damp"] if _hit(name, rule)]
    assert len(factors) <= 1, name
    return factors[0] if factors else 1.0


def _sd_of(tag):
    """state_dict under the generator's rules, each of which must hit something."""
    meta = fixture(tag)[1]
    for rule in meta["damp"]:
        assert any(_hit(n, rule) for n, _ in meta["names"]), rule
    return state_dict(tag, _damp)


def _hw(dtype):
    return F16 if dtype == "fp16" else F32


# ---- host side (no GPU) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_stock_cfg_is_the_reference_yaml(scale):
    for tag in GRAPHS:
        want = dict(fixture(tag)[1]["yaml"])
        assert [l[3] for l in want["head"] if l[2] == "nn.Upsample"][0] == ["None", 2, "nearest"]  # yaml's string; parse_model evaluates it (tasks.py:981-985)
        want["head"] = [[f, n, m, [None if a == "None" else a for a in args]] for f, n, m, args in want["head"]]
        assert want["nc"] == 80 and "scale" not in want and want["head"][-1][2] == "WorldDetect"
        cfg = stock_cfg("yolov8-worldv2", scale, 80)
        assert cfg.pop("scale") == scale and cfg == want
    for bad in (dict(scale="t"), dict(scale=None), dict(scale="n", task="segment"), dict(scale="n", task="classify"), dict(scale="n", task="obb")):
        with pytest.raises(ValueError):
            stock_cfg("yolov8-worldv2", bad["scale"], 80, bad.get("task", "detect"))
    with pytest.raises(ValueError):
        stock_cfg("yolov8-worldv2", "n", 1, "pose", kpt_shape=(17, 3))
    cfg = stock_cfg("yolov8-worldv2", scale, 80)
    cfg["head"][2][3][0] = 7  # a deep copy: the table is not the caller's to change
    assert stock_cfg("yolov8-worldv2", scale, 80)["head"][2][3] == [512, 256, 8]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("scale", SCALES)
def test_world_plans(scale, precision):
    """Every scale plans in every precision at 64 x 64 and 96 x 128: exactly four MAXSIG ops, each directly behind a 3x3 CONV with act = 0 whose
    destination is the MAXSIG's src1 and dst, its embedding the chunk before; meta and the outputs follow text_nc."""
    from bs_yolo_amd.plugin import SUPPORTED_HEADS, graph_support, max_stride
    cfg = stock_cfg("yolov8-worldv2", scale, 80)
    assert "WorldDetect" in SUPPORTED_HEADS and graph_support(cfg) == {"fp16": True, "fp32": True} and max_stride(cfg) == 32
    width, max_ch = cfg["scales"][scale][1:]
    for (h, w), tnc in (((64, 64), None), ((96, 128), 12), ((64, 64), 1203)):
        plan = Plan(cfg, 2, h, w, precision=precision, text_nc=tnc)
        nc = tnc or 80
        m = plan.meta
        assert m["nc"] == nc and m["no"] == 64 + nc and m["world"] is True and m.get("task", "detect") == "detect" and m["legacy"]
        assert m["strides"] == [8.0, 16.0, 32.0] and m["levels"] == [(h // s, w // s) for s in (8, 16, 32)]
        A = sum(lh * lw for lh, lw in m["levels"])
        assert plan.outputs["y"].shape == (2, 4 + nc, A)
        assert [plan.outputs[f"raw{l}"].shape for l in range(3)] == [(2, 64 + nc, lh, lw) for lh, lw in m["levels"]]
        ms = kinds(plan, L.OP_MAXSIG)
        assert len(ms) == 4 and [o["name"] for o in ms] == [f"model.{i}.attn" for i in ATTN]
        for o, i in zip(ms, ATTN):
            prev = plan.ops[plan.ops.index(o) - 1]
            assert prev["kind"] == L.OP_CONV and prev["ksize"] == 3 and prev["act"] == 0 and prev["name"] == f"model.{i}.attn.proj_conv"
            assert prev["dst"] is o["src1"] and o["dst"] is o["src1"] and prev["src0"] is o["src0"] and prev.get("res") is None
            c = o["heads"] * o["head_dim"]
            assert o["head_dim"] == 32 and o["nc"] == nc and o["src0"].C == o["dst"].C == c and o["src0"].buf == o["dst"].buf
            assert o["dst"].coff == o["src0"].coff + c  # the chunk behind the embedding's
            c2 = -(-min(cfg["head"][i - 10][3][0], max_ch) * width // 8) * 8
            assert c == c2 // 2 and plan.layer_out[i].C == c2
            r = plan.wrecs[o["wkey"]]
            assert (r.kind, r.name, r.cout, r.cin, r.k, r.embed) == ("maxsig", f"model.{i}.attn", nc, c, o["heads"], 512)
            nxt = plan.ops[plan.ops.index(o) + 1]  # cv2 over every chunk
            n = max(round(3 * cfg["scales"][scale][0]), 1)
            assert nxt["name"] == f"model.{i}.cv2" and nxt["src0"].C == (3 + n) * c and nxt["src0"].buf == o["dst"].buf
        if scale in HEADS:
            assert [o["heads"] for o in ms] == HEADS[scale]
        for l in range(3):
            r = plan.wrecs[f"model.22.cv3.{l}.2"]
            assert (r.kind, r.cout, r.post, r.embed) == ("world_cls", nc, f"model.22.cv4.{l}", 512)
        assert {r.kind for r in plan.wrecs.values()} == {"conv", "first", "plain", "maxsig", "world_cls"}
        if tnc != 1203:
            Wt.pack_plan_weights(plan, Wt.synth_state_dict(plan))
            ops = plan.c_ops()
            assert [(o.heads, o.head_dim, o.nc) for o in ops if o.kind == L.OP_MAXSIG] == [(o["heads"], 32, nc) for o in ms]


def test_fixture_plans_flops_and_weight_names():
    """The fixtures' graphs: the dense convs' FLOPs against the reference's count (the folded head counted as folded); packing reads every
    parameter name the reference's model holds but the DFL conv and num_batches_tracked, un-fused and after fuse()-style folding alike."""
    t1, _ = _texts()
    for tag in GRAPHS:
        meta = fixture(tag)[1]
        sd = _sd_of(tag)
        assert meta["heads"] == HEADS[meta["scale"]] and meta["hc"] == [32] * 4 and meta["n"] == [2 if meta["scale"] == "m" else 1] * 4
        assert meta["bn_eps"] == Wt.BN_EPS and meta["stride"] == [8.0, 16.0, 32.0]
        r = meta["ref_fp16"]  # the conditions the generator checked
        assert r["score"] < 5e-3 and r["box"] < 0.5 and r["raw"] < 1.5e-2 and r["layer_max"] < 256
        assert all(g[0] < 0.25 and g[1] > 0.75 for g in meta["gate"].values()) and all(lo < 0.01 and hi > 0.25 for lo, hi in meta["score_range"])
        assert all(v >= 2.0 for v in meta["class_spread"].values())  # the classes matter: a wrong maximum moves a gate's logit by 2 or more somewhere
        # fuse()-style: BaseModel.fuse folds the Convs it recognises -- the top-level ones and the head's; block.py's own Conv (C2f, C2fAttn, SPPF) keeps its BN
        fused = dict(sd)
        for n in [n for n in sd if n.endswith(".conv.weight") and (re.fullmatch(r"model\.\d+\.conv\.weight", n) or n.startswith("model.22.cv"))]:
            p = n[:-len(".conv.weight")]
            w, b = Wt.fold_conv_bn(sd, p)
            fused[p + ".conv.weight"], fused[p + ".conv.bias"] = w, b
            for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
                fused.pop(f"{p}.bn.{k}", None)
        assert len(fused) < len(sd) and "model.12.attn.proj_conv.bn.weight" in fused and "model.0.bn.weight" not in fused
        for precision in PRECISIONS:
            for si, (b, h, w) in enumerate(meta["shapes"]):
                plan = Plan(cfg_of(meta), b, h, w, precision=precision)
                dense = sum(o.get("mfma_flops", 0) for o in plan.ops if o["kind"] != L.OP_MAXSIG)
                assert abs(dense - meta["conv_flops"][si]) <= 0.01 * meta["conv_flops"][si], (tag, precision, si, dense, meta["conv_flops"][si])
                gate = sum(2 * b * o["H"] * o["W"] * o["src0"].C * NC for o in kinds(plan, L.OP_MAXSIG))
                assert plan.flops >= dense + gate
            skip = lambda n: n.endswith(".dfl.conv.weight") or n.endswith("num_batches_tracked")  # noqa: E731
            blobs = []
            for form in (sd, fused):
                seen = set()

                class Recording(dict):
                    def __getitem__(self, k):
                        seen.add(k)
                        return dict.__getitem__(self, k)

                plan = Plan(cfg_of(meta), 1, 64, 64, precision=precision)
                blobs.append(Wt.pack_plan_weights(plan, Recording(dict(form, txt_feats=t1))))
                assert seen == {n for n in form if not skip(n)} | {"txt_feats"}, (tag, precision, sorted(seen ^ {n for n in form if not skip(n)})[:6])
                assert len(plan.c_ops()) == len(plan.ops)
            assert len(blobs[0]) == len(blobs[1])
            assert set(Wt.synth_state_dict(plan)) == {n for n in sd if not skip(n)} | {"txt_feats"}


def test_text_nc_and_cfg_nc():
    """text_nc = 5 with cfg["nc"] = 80 keeps c3 = max(ch0, min(80, 100)) (head.py:313); cfg["nc"] = 12 gives max(ch0, 12)."""
    cfg = stock_cfg("yolov8-worldv2", "n", 80)
    for precision in PRECISIONS:
        plan = Plan(cfg, 1, 64, 64, precision=precision, text_nc=5)
        ch0 = plan.layer_out[15].C
        assert ch0 == 64 and plan.meta["nc"] == 5 and plan.outputs["y"].shape == (1, 9, 84) and plan.outputs["raw0"].shape == (1, 69, 8, 8)
        for l in range(3):
            assert plan.wrecs[f"model.22.cv3.{l}.0"].cout == 80 and plan.wrecs[f"model.22.cv3.{l}.1"].cout == 80
            r = plan.wrecs[f"model.22.cv3.{l}.2"]
            assert (r.cout, r.cin) == (5, 80)
        p12 = Plan(stock_cfg("yolov8-worldv2", "n", 12), 1, 64, 64, precision=precision, text_nc=5)
        assert p12.wrecs["model.22.cv3.0.0"].cout == 64 and p12.wrecs["model.22.cv3.0.2"].cin == 64 and p12.meta["nc"] == 5
    p100 = Plan(stock_cfg("yolov8-worldv2", "n", 1203), 1, 64, 64)  # c3 = 100: carried on 104 channels, as the legacy Detect head does
    r = p100.wrecs["model.22.cv3.0.2"]
    assert (r.cout, r.cin, r.real_cin) == (1203, 104, 100)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="text_nc"):
            Plan(cfg, 1, 64, 64, text_nc=bad)
    with pytest.raises(ValueError, match="WorldDetect"):
        Plan(stock_cfg("yolov8", "n", 80), 1, 64, 64, text_nc=5)


def test_refusals():
    from bs_yolo_amd.plugin import graph_support
    base = stock_cfg("yolov8-worldv2", "n", 80)
    # yolov8-world.yaml (v1): an ImagePoolingAttn layer between the neck's halves
    v1 = copy.deepcopy(base)
    v1["head"].insert(6, [[15, 12, 9], 1, "ImagePoolingAttn", [256]])
    with pytest.raises(NotImplementedError, match=r"model\.16: ImagePoolingAttn is not accelerated: YOLO-World v1"):
        Plan(v1, 1, 64, 64)
    assert graph_support(v1) == {"fp16": False, "fp32": False}
    # ContrastiveHead: with_bn False, or left out (the constructor's default)
    for args in (["nc", 512, False], ["nc", 512], ["nc"]):
        c = copy.deepcopy(base)
        c["head"][-1][3] = args
        for precision in PRECISIONS:
            with pytest.raises(NotImplementedError, match=r"model\.22: WorldDetect with with_bn = False .*not linear"):
                Plan(c, 1, 64, 64, precision=precision)
    # a C2fAttn under another head
    c = copy.deepcopy(base)
    c["head"][-1] = [[15, 18, 21], 1, "Detect", ["nc"]]
    with pytest.raises(NotImplementedError, match=r"model\.12: C2fAttn in a graph whose head is Detect, not WorldDetect"):
        Plan(c, 1, 64, 64)
    assert graph_support(c) == {"fp16": False, "fp32": False}
    # ReLU graphs hold convs alone
    with pytest.raises(NotImplementedError, match=r"model\.2: C2f under activation nn\.ReLU\(\)"):
        Plan(dict(base, activation="nn.ReLU()"), 1, 64, 64)
    # heads the fp16 kernel does not take: 16 heads on layer 15's 32 channels at scale n -> int(16 * 0.25) = 4 heads of hc = 8
    c = copy.deepcopy(base)
    c["head"][5][3] = [256, 128, 16]
    with pytest.raises(NotImplementedError, match=r"model\.15: C2fAttn heads of hc = 8 channels are not on the fp16 path"):
        Plan(c, 1, 64, 64)
    p = Plan(c, 1, 64, 64, precision="fp32")
    assert [(o["heads"], o["head_dim"]) for o in kinds(p, L.OP_MAXSIG)][1] == (4, 8) and graph_support(c) == {"fp16": False, "fp32": True}
    c["head"][5][3] = [256, 128, 12]  # 3 heads on 32 channels
    with pytest.raises(NotImplementedError, match=r"model\.15: C2fAttn with 3 heads on 32 channels"):
        Plan(c, 1, 64, 64, precision="fp32")
    c["head"][5][3] = [256, 256, 4]  # ec = 64 != c = 32: attn.ec
    with pytest.raises(NotImplementedError, match=r"model\.15: C2fAttn with ec = 64 != c = 32"):
        Plan(c, 1, 64, 64, precision="fp32")
    c = copy.deepcopy(base)
    c["head"].append([-1, 1, "Conv", [64, 1, 1]])
    with pytest.raises(NotImplementedError):  # (not the last layer: C2fAttn's own check sees another head first)
        Plan(c, 1, 64, 64)


def _rand(g, *shape, scale=1.0, shift=0.0):
    return (torch.rand(*shape, generator=g, dtype=F64) * 2 - 1) * scale + shift


def test_maxsig_record_is_the_modules_formula():
    """G[n] = (gl.weight @ t_n + gl.bias) / sqrt(hc) with t_n as given (not normalised), [bias | scale] behind it; the f16 form padded to 32
    rows with copies of row 0."""
    g = torch.Generator().manual_seed(3)
    for nc, nh, hc, with_scale in ((12, 2, 32, False), (33, 3, 16, True), (64, 1, 48, False), (1, 4, 8, True)):
        c = nh * hc
        t = _rand(g, 1, nc, E, scale=2.0)  # (1, nc, E), rows of any length
        sd = {"a.gl.weight": _rand(g, c, E), "a.gl.bias": _rand(g, c), "a.bias": _rand(g, nh), "txt_feats": t}
        scale = torch.ones(nh, dtype=F64)
        if with_scale:
            sd["a.scale"] = _rand(g, 1, nh, 1, 1, shift=1.5)
            scale = sd["a.scale"].reshape(-1)
        sd32 = {k: v.float() for k, v in sd.items()}  # what a state dict holds
        want = torch.stack([(sd32["a.gl.weight"].double() @ t[0, n].float().double() + sd32["a.gl.bias"].double()) / math.sqrt(hc) for n in range(nc)])
        r = WRec(name="a", kind="maxsig", cout=nc, cin=c, k=nh)
        r.embed = E
        wb, bb = Wt.pack_record(sd32, r, f32=True)
        G32 = np.frombuffer(wb, np.float32).reshape(nc, c)
        np.testing.assert_allclose(G32, want.numpy(), rtol=1e-6, atol=1e-30)
        bs = np.frombuffer(bb, np.float32)
        np.testing.assert_allclose(bs, torch.cat([sd32["a.bias"].double(), scale.float().double()]).numpy(), rtol=1e-6)
        wb16, bb16 = Wt.pack_record(sd32, r, f32=False)
        rows = -(-nc // 32) * 32
        G16 = np.frombuffer(wb16, np.float16).reshape(rows, c)
        assert np.array_equal(G16[:nc], want.numpy().astype(np.float16)) or np.allclose(G16[:nc].astype(np.float64), want.numpy(), rtol=2.0 ** -10, atol=2.0 ** -24)
        assert all(np.array_equal(G16[j], G16[0]) for j in range(nc, rows)) and bb16 == bb
        assert set(Wt.record_keys(r)) == {"a.gl.weight", "a.gl.bias", "a.bias", "txt_feats"}
    with pytest.raises(ValueError, match="rows of E = 512"):
        Wt.pack_record(dict(sd32, txt_feats=torch.zeros(1, 256)), r)
    with pytest.raises(ValueError, match="has 3 rows, the plan was built to score 1"):
        Wt.pack_record(dict(sd32, txt_feats=torch.zeros(3, E)), r)
    with pytest.raises(NotImplementedError, match="per-image text features"):
        Wt.pack_record(dict(sd32, txt_feats=torch.zeros(2, 1, E)), r)
    with pytest.raises(KeyError, match="txt_feats"):
        Wt.pack_record({k: v for k, v in sd32.items() if k != "txt_feats"}, r)


def test_world_cls_record_is_the_modules_formula():
    """BNContrastiveHead(cv3.l.2(x), text) written out -- the 1x1 conv, the eval-mode BatchNorm, F.normalize of the text rows, the einsum,
    exp(logit_scale), the bias -- against the ONE biased 1x1 conv the record holds, in the fp32 layout (K x cout) and through the padded
    input width the legacy head uses for c3 = 100."""
    g = torch.Generator().manual_seed(4)
    eps = 1e-3
    for nc, c3, c3p in ((12, 64, 64), (5, 100, 104), (40, 80, 80)):
        sd = {"h.cv3.1.2.weight": _rand(g, E, c3, 1, 1), "h.cv3.1.2.bias": _rand(g, E), "h.cv4.1.norm.weight": _rand(g, E, scale=1.5),
              "h.cv4.1.norm.bias": _rand(g, E), "h.cv4.1.norm.running_mean": _rand(g, E), "h.cv4.1.norm.running_var": _rand(g, E, scale=0.5, shift=1.0),
              "h.cv4.1.bias": _rand(g, 1, shift=-3.0), "h.cv4.1.logit_scale": _rand(g, 1).reshape(()), "txt_feats": _rand(g, nc, E, scale=3.0)}
        sd = {k: v.float() for k, v in sd.items()}
        d = {k: v.double() for k, v in sd.items()}

        def module(X):  # X (n, c3) pixels -> (n, nc) class logits, as the reference's modules compute them
            emb = X @ d["h.cv3.1.2.weight"].flatten(1).t() + d["h.cv3.1.2.bias"]
            xn = (emb - d["h.cv4.1.norm.running_mean"]) / torch.sqrt(d["h.cv4.1.norm.running_var"] + eps) * d["h.cv4.1.norm.weight"] + d["h.cv4.1.norm.bias"]
            wn = d["txt_feats"] / d["txt_feats"].norm(dim=-1, keepdim=True)
            return torch.einsum("pc,kc->pk", xn, wn) * torch.exp(d["h.cv4.1.logit_scale"]) + d["h.cv4.1.bias"]

        b_ref = module(torch.zeros(1, c3, dtype=F64))[0]
        W_ref = (module(torch.eye(c3, dtype=F64)) - b_ref).t()  # (nc, c3)
        r = WRec(name="h.cv3.1.2", kind="world_cls", cout=nc, cin=c3p, k=1, real_cin=c3 if c3p != c3 else 0, post="h.cv4.1")
        r.embed = E
        wb, bb = Wt.pack_record(sd, r, eps, f32=True)
        Wm = np.frombuffer(wb, np.float32).reshape(c3p, nc)
        np.testing.assert_allclose(Wm[:c3].T, W_ref.numpy(), rtol=1e-6, atol=1e-9 * float(W_ref.abs().max()))
        assert not Wm[c3:].any()
        np.testing.assert_allclose(np.frombuffer(bb, np.float32), b_ref.numpy(), rtol=1e-6, atol=1e-9)
        wb16, bb16 = Wt.pack_record(sd, r, eps, f32=False)
        cp, kp = Wt.packed_dims(nc, c3p, 1)
        W16 = np.frombuffer(wb16, np.float16).reshape(cp, kp)
        assert np.allclose(W16[:nc, :c3].astype(np.float64), W_ref.numpy(), rtol=2.0 ** -10, atol=2.0 ** -24) and not W16[nc:].any() and not W16[:, c3:].any()
        np.testing.assert_allclose(np.frombuffer(bb16, np.float32)[:nc], b_ref.numpy(), rtol=1e-6, atol=1e-9)
        assert set(Wt.record_keys(r)) == set(sd)
    with pytest.raises(ValueError, match="rows of E = 512"):
        Wt.pack_record(dict(sd, txt_feats=torch.zeros(nc, 384)), r)
    with pytest.raises(ValueError, match="has 7 rows"):
        Wt.pack_record(dict(sd, txt_feats=torch.zeros(7, E)), r)


def test_maxsig_is_declared_and_checks_its_arguments():
    header = (ROOT / "include" / "bsyolo.h").read_text()
    assert "bsy_maxsig_attn(" in header and "BSY_OP_MAXSIG = 29" in header and "bsy_maxsig_supported(" in header
    assert {"bsy_maxsig_attn", "bsy_maxsig_supported"} <= set(L.SYMBOLS) and L.OP_MAXSIG == 29
    assert [hc for hc in range(0, 200) if L.lib.bsy_maxsig_supported(hc)] == list(range(16, 129, 16))
    f = L.lib.bsy_maxsig_attn
    d, e, o = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(1 << 20)  # never dereferenced: every check below fails before a launch

    def call(embed=e, lde=64, proj=d, ldp=64, out=o, ldo=64, B=1, H=3, W=5, heads=2, hc=32, G=d, nc=12, bs=d, dtype=L.BSY_F16):
        return f(embed, lde, proj, ldp, out, ldo, B, H, W, heads, hc, G, nc, bs, dtype, None)

    for k in ("embed", "proj", "out", "G", "bs"):
        with pytest.raises(L.BsyError, match="maxsig: null pointer"):
            L.check(call(**{k: None}))
    for nc in (0, -3):
        with pytest.raises(L.BsyError, match=r"maxsig: nc = %d" % nc):
            L.check(call(nc=nc))
    for hc in (8, 24, 144, 0):
        with pytest.raises(L.BsyError, match="maxsig: heads of hc = %d channels are not on the fp16 path" % hc if hc else "maxsig: 1 images"):
            L.check(call(hc=hc, lde=512, ldp=512, ldo=512))
    with pytest.raises(L.BsyError, match="overlaps the embedding"):
        L.check(call(out=e))  # the embedding itself
    with pytest.raises(L.BsyError, match="overlaps the embedding"):
        L.check(call(out=C.c_void_p(8192 + 2 * 32), lde=128, ldo=128))  # one buffer, channel windows [0, 64) and [32, 96)
    with pytest.raises(L.BsyError, match="overlaps the embedding"):
        L.check(call(out=C.c_void_p(8192 + 16), lde=64, ldo=72))  # different strides inside one address range
    with pytest.raises(L.BsyError, match="row strides"):
        L.check(call(ldp=56))
    with pytest.raises(L.BsyError, match="multiples of 8 and 16-byte aligned"):
        L.check(call(lde=68))
    with pytest.raises(L.BsyError, match="multiples of 8 and 16-byte aligned"):
        L.check(call(proj=C.c_void_p(4104)))
    with pytest.raises(L.BsyError, match="dtype 2"):
        L.check(call(dtype=L.BSY_U8))
    with pytest.raises(L.BsyError, match="bad map size"):
        L.check(call(H=0))
    with pytest.raises(L.BsyError, match="f32: 4-byte"):
        L.check(call(dtype=L.BSY_F32, hc=7, heads=3, proj=C.c_void_p(4098)))


# ------------------------------------------------------------------------------------------------------------
# MAXSIG alone
# ------------------------------------------------------------------------------------------------------------
MAPS = ((3, 5), (9, 21))
HEAD_SHAPES = ((1, 32), (3, 32), (2, 64), (4, 16))
NCS = (1, 12, 31, 32, 33, 100)
BIG_NC = 1203
MS_B = 2


def _maxsig_op(prec, B, H, W, nh, hc, nc, src0, src1, dst, w_off, b_off):
    op = new_op(L.OP_MAXSIG, prec, B, H, W)
    op.src0, op.src1, op.dst = src0, src1, dst
    op.heads, op.head_dim, op.nc, op.w_off, op.b_off = nh, hc, nc, w_off, b_off
    return op


def _payload(kind, g, B, H, W, nh, hc, nc, dt):
    """(embedding, guide (nc, C), bias (nh)) as float64 tensors holding values exact in `dt`; the guide carries its own gain."""
    Cc = nh * hc
    if kind == "dyadic":
        e = torch.randint(-16, 17, (B, H, W, Cc), generator=g).double() / 8
        G = torch.randint(-2, 3, (nc, Cc), generator=g).double() / 2 * (torch.rand(nc, Cc, generator=g) < 0.15)
        bias = torch.zeros(nh, dtype=F64)
    elif kind == "negative":  # every real class scores below zero on every pixel: a zero-padded guide row would win the maximum
        e = torch.randint(1, 17, (B, H, W, Cc), generator=g).double() / 8
        G = torch.zeros(nc, Cc, dtype=F64)
        for m in range(nh):
            idx = torch.stack([torch.randperm(hc, generator=g)[:3] for _ in range(nc)]) + m * hc
            G.scatter_(1, idx, -torch.randint(1, 3, (nc, 3), generator=g).double() / 2)
        bias = torch.randint(0, 9, (nh,), generator=g).double() / 8
    else:
        e = torch.randn(B, H, W, Cc, generator=g).to(dt).double()
        G = (torch.randn(nc, Cc, generator=g) / math.sqrt(hc)).to(dt).double()
        bias = torch.randn(nh, generator=g).float().double()
    return e, G, bias


def _dots(e, G, nh, hc):
    """(t = max_n <e, G_n> per (pixel, head), S = max_n sum_k |e_k G_nk|), float64 (B, H, W, nh).  No partial sum of a dot product, in any
    order, exceeds S."""
    B, H, W, Cc = e.shape
    eh, Gh = e.reshape(B, H, W, nh, hc), G.reshape(-1, nh, hc)
    dots = torch.einsum("bhwmk,nmk->bhwnm", eh, Gh)
    mags = torch.einsum("bhwmk,nmk->bhwnm", eh.abs(), Gh.abs())
    return dots.max(dim=3)[0], mags.max(dim=3)[0]


def _run_maxsig(prec, e, proj, G, bias, scale, nh, hc, inplace):
    """One MAXSIG op on poisoned views -> (the destination view as stored, bits untouched elsewhere asserted here)."""
    dt = F32 if prec else F16
    B, H, W, Cc = e.shape
    nc = G.shape[0]
    lde, ce, ldp, cp, ldd, cd = Cc + 24, 8, Cc + 24, 16, Cc + 16, 8
    te = poisoned((B, H, W, lde), ce, Cc, e.to(dt), NAN)
    tp = poisoned((B, H, W, ldp), cp, Cc, proj.to(dt), NAN)
    td = None if inplace else poisoned((B, H, W, ldd), cd, Cc, None, POISON32 if prec else POISON16, dt)
    Gp = Wt.guide(G, bool(prec))
    assert Gp.shape[0] == (nc if prec else -(-nc // 32) * 32) and (prec or all(torch.equal(Gp[j], Gp[0]) for j in range(nc, Gp.shape[0])))
    assert torch.equal(Gp[:nc].double(), G)  # the payload's values are exact in the storage type
    blob, (w_off, b_off) = poisoned_blob([Gp.numpy(), torch.cat([bias, scale]).float().numpy()])
    dst = view(1, ldp, cp, Cc) if inplace else view(2, ldd, cd, Cc)
    op = _maxsig_op(prec, B, H, W, nh, hc, nc, view(0, lde, ce, Cc), view(1, ldp, cp, Cc), dst, w_off, b_off)
    before = [t.cpu().clone() for t in (te, tp)] + ([td.cpu().clone()] if td is not None else [])
    run_ops([op], [te, tp, td], blob)
    assert torch.equal(bits(te), bits(before[0]))  # src0 keeps its bits
    if inplace:
        assert_outside_views_intact(tp, before[1], [(cp, Cc)])
        return tp[..., cp:cp + Cc].cpu()
    assert torch.equal(bits(tp), bits(before[1]))  # ... and src1, out of place
    assert_outside_views_intact(td, before[2], [(cd, Cc)])
    return td[..., cd:cd + Cc].cpu()


def _check_maxsig(prec, kind, H, W, nh, hc, nc, inplace, g):
    dt = F32 if prec else F16
    B = MS_B
    e, G, bias = _payload(kind, g, B, H, W, nh, hc, nc, dt)
    t, S = _dots(e, G, nh, hc)
    if kind == "dyadic":  # centre the gates: the median maximum of a head, in eighths, goes into its bias
        bias = -(t.reshape(-1, nh).median(dim=0)[0] * 8).round() / 8
    if kind == "negative":
        assert float(t.max()) < 0
    if kind != "random":
        assert float(S.max()) < 2 ** 10 and bool(((e * 8) == (e * 8).round()).all()) and bool(((G * 2) == (G * 2).round()).all()) and float(e.abs().max()) <= 2
    proj = torch.randn(B, H, W, nh * hc, generator=g).to(dt).double()
    scale = torch.tensor([1.0, 0.75, 1.5, 1.25][:nh], dtype=F64)
    tt = t + bias
    gate = (scale / (1 + torch.exp(-tt))).repeat_interleave(hc, dim=-1)  # (B, H, W, C)
    ref = proj * gate
    got = _run_maxsig(prec, e, proj, G, bias, scale, nh, hc, inplace).double()
    assert bool(torch.isfinite(got).all()), (kind, "a NaN from outside a view or between the records reached the output")
    rnd = torch.from_numpy(ulp32(ref.numpy())) * 0.5 if prec else torch.from_numpy(ulp16(ref.numpy())) * 0.5
    if kind == "random":
        dtt = (1.1 * hc * U * S + U * tt.abs()).repeat_interleave(hc, dim=-1)
        bound = (proj * scale.repeat_interleave(hc)).abs() * dtt / 4 + 8 * U * ref.abs() + rnd
    elif prec:
        bound = 8 * U * ref.abs() + torch.from_numpy(ulp32(ref.numpy()))
    else:
        bound = torch.from_numpy(ulp16(ref.numpy()))
    worst = float(((got - ref).abs() / bound).max())
    lo, hi = float(gate.min()), float(gate.max())
    print(f"maxsig prec {prec} {kind} {H}x{W} heads {nh} x {hc} nc {nc} {'in place' if inplace else 'out of place'}: worst |got - ref| / bound "
          f"{worst:.3f}, gates {lo:.3f} .. {hi:.3f}")
    assert worst <= 1.0, (kind, prec, H, W, nh, hc, nc, inplace, worst)
    if kind == "negative" and nc % 32:  # what a zero-padded guide would have returned is far outside the bound
        wrong = proj * (scale / (1 + torch.exp(-t.clamp(min=0) - bias))).repeat_interleave(hc, dim=-1)
        assert float(((wrong - ref).abs() / bound).max()) > 100
    if not inplace:  # batch independence: each image alone returns the bits it has inside the batch
        for b in range(B):
            alone = _run_maxsig(prec, e[b:b + 1], proj[b:b + 1], G, bias, scale, nh, hc, False)
            assert torch.equal(bits(alone.to(dt)), bits(got[b:b + 1].to(dt))), (kind, "image", b)
    return lo, hi


@gpu
@pytest.mark.parametrize("nh,hc", HEAD_SHAPES, ids=[f"{a}x{b}" for a, b in HEAD_SHAPES])
@pytest.mark.parametrize("prec", [0, 1, 2], ids=["fp16", "fp32", "fp32x"])
def test_maxsig_op(prec, nh, hc):
    g = torch.Generator().manual_seed(1000 * prec + 10 * nh + hc)
    spread = [1.0, 0.0]
    for hi, (H, W) in enumerate(MAPS):
        for nc in NCS + ((BIG_NC,) if hi == 1 else ()):
            for inplace in (False, True):
                if prec == 2 and (inplace or nc in (31, 100)):  # fp32x runs the fp32 kernel: one pass over the class counts, out of place
                    continue
                for kind in ("dyadic", "negative", "random"):
                    if nc == BIG_NC and (kind == "negative" or inplace):
                        continue
                    lo, hi_ = _check_maxsig(prec, kind, H, W, nh, hc, nc, inplace, g)
                    if kind == "dyadic":
                        spread = [min(spread[0], lo), max(spread[1], hi_)]
    assert spread[0] < 0.25 and spread[1] > 0.6, spread  # the dyadic gates are not all at one end


def _create(ops):
    """bsy_plan_create alone on a list of ops -> (status, message); the plan, if any, is destroyed."""
    blob = b"\0" * 256
    eng, plan = C.c_void_p(), C.c_void_p()
    L.check(L.lib.bsy_engine_create(0, C.byref(eng)))
    try:
        L.check(L.lib.bsy_engine_load_weights(eng, (C.c_char * len(blob)).from_buffer_copy(blob), len(blob)))
        rc = L.lib.bsy_plan_create(eng, (L.Op * len(ops))(*ops), len(ops), None, 0, C.byref(plan))
        msg = L.lib.bsy_last_error().decode(errors="replace") if rc else ""
    finally:
        if plan:
            L.lib.bsy_plan_destroy(plan)
        L.lib.bsy_engine_destroy(eng)
    return rc, msg


@gpu
def test_plan_creation_refuses_a_bad_maxsig_record():
    def op(prec=0, nh=2, hc=32, nc=12, src0=view(0, 96, 8, 64), src1=view(1, 96, 16, 64), dst=view(2, 96, 8, 64)):
        return _maxsig_op(prec, 1, 3, 5, nh, hc, nc, src0, src1, dst, 0, 0)

    assert _create([op()])[0] == 0 and _create([op(dst=view(1, 96, 16, 64))])[0] == 0  # out of place, in place
    from op_plan_helpers import no_view
    for bad, text in ((dict(src0=no_view()), "null pointer"), (dict(src1=no_view()), "null pointer"), (dict(dst=no_view()), "null pointer"),
                      (dict(nc=0), "nc = 0"), (dict(hc=8, src0=view(0, 96, 8, 16), src1=view(1, 96, 16, 16), dst=view(2, 96, 8, 16)), "hc = 8"),
                      (dict(dst=view(0, 96, 8, 64)), "overlaps the embedding"), (dict(src0=view(0, 160, 8, 64), dst=view(0, 160, 40, 64)), "overlaps the embedding"),
                      (dict(src1=view(1, 96, 16, 32)), "2 heads of 32 channels on views of 64 / 32 / 64")):
        rc, msg = _create([new_op(L.OP_COPY, 0, 1, 4, 4), op(**bad)])
        assert rc != 0 and "op 1 (MAXSIG)" in msg and text in msg, (bad, msg)
    assert _create([op(prec=1, hc=8, src0=view(0, 96, 8, 16), src1=view(1, 96, 16, 16), dst=view(2, 96, 8, 16))])[0] == 0  # the fp32 modes take any hc
    assert _create([op(src0=view(0, 160, 8, 64), dst=view(0, 160, 72, 64))])[0] == 0  # one buffer, disjoint channel windows


@gpu
def test_ops_maxsig_attn_wrapper():
    """ops.maxsig_attn on channel slices of wider tensors, in place and into a new tensor, against float64."""
    from bs_yolo_amd import ops as O
    g = torch.Generator().manual_seed(5)
    for dt, nh, hc, nc in ((F16, 2, 32, 12), (F32, 3, 20, 7)):
        Cc = nh * hc
        wide = torch.randn(2, 5, 7, 2 * Cc + 16, generator=g).to(dt).to(DEV)
        e, p = wide[..., 8:8 + Cc], wide[..., Cc + 16:]
        G = (torch.randn(nc, Cc, generator=g) / math.sqrt(hc)).to(dt)
        bias, scale = torch.randn(nh, generator=g), torch.tensor([1.0, 0.5, 2.0][:nh])
        t = (e.cpu().double().view(2, 5, 7, 1, nh, hc) * G.double().view(nc, nh, hc)).sum(-1).max(dim=3)[0] + bias.double()
        ref = p.cpu().double() * (scale.double() / (1 + torch.exp(-t))).repeat_interleave(hc, dim=-1)
        tol = 2.0 ** -9 if dt == F16 else 1e-5
        out = O.maxsig_attn(e, p, G, bias, scale, nh)
        torch.cuda.synchronize()
        assert out.shape == p.shape and out.dtype == dt and float((out.cpu().double() - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max()))
        same = O.maxsig_attn(e, p, G, bias, scale, nh, out=p)
        torch.cuda.synchronize()
        assert same.data_ptr() == p.data_ptr() and torch.equal(bits(p), bits(out))
        with pytest.raises(L.BsyError, match="overlaps the embedding"):
            O.maxsig_attn(e, p, G, bias, scale, nh, out=e)


# ------------------------------------------------------------------------------------------------------------
# the graphs
# ------------------------------------------------------------------------------------------------------------
def _engine(tag, precision, txt=None, **kw):
    from bs_yolo_amd.engine import YoloEngine
    return YoloEngine(cfg_of(fixture(tag)[1]), _sd_of(tag), precision=precision, txt_feats=_texts()[0] if txt is None else txt, **kw)


def _compare(eng, z, meta, precision, nc, ykey, rawkey, what, nms=True):
    from bs_yolo_amd import nms as HN
    from oracle import postproc_ref as PP
    kept = 0
    for si, (b, h, w) in enumerate(meta["shapes"]):
        x = x_of(meta, si)
        y, raws = eng((x.half() if precision == "fp16" else x).to(DEV))
        torch.cuda.synchronize()
        plan = eng.plan_for(b, h, w, *(2 * [_hw(precision)]))[0]
        assert len(kinds(plan, L.OP_MAXSIG)) == 4 and plan.meta["nc"] == nc
        levels = [(h // int(s), w // int(s)) for s in meta["stride"]]
        assert tuple(y.shape) == (b, 4 + nc, sum(lh * lw for lh, lw in levels)) and len(raws) == len(levels)
        assert [tuple(r.shape) for r in raws] == [(b, 64 + nc, lh, lw) for lh, lw in levels]
        yr = y.float().cpu().numpy()
        assert np.isfinite(yr).all()
        check_y(yr, z[ykey % si], meta["stride"], level_of_anchor(levels), max(h, w), precision, f"{what} shape {si}", nc, Y_BOUNDS)
        for l, r in enumerate(raws):
            check_raw(r.float().cpu().numpy(), z[rawkey % (si, l)], precision, f"{what} shape {si} raw {l}", RAW_BOUNDS)
        if not nms:
            continue
        conf, iou = meta["nms_conf"], meta["nms_iou"]
        pinned = HN.non_max_suppression(torch.from_numpy(z[ykey % si]).to(DEV), conf, iou, nc=nc)
        mine = HN.non_max_suppression(y.float().clone(), conf, iou, nc=nc)  # (both convert xywh in place)
        oracle = PP.non_max_suppression(y.float().cpu().clone(), conf, iou, nc=nc)
        for bi in range(b):
            want = z[f"nms{si}_{bi}"]
            assert tuple(pinned[bi].shape) == want.shape and np.allclose(pinned[bi].cpu().numpy(), want, atol=1e-5, rtol=0), (what, si, bi)
            assert torch.equal(mine[bi].cpu(), oracle[bi]), (what, si, bi)
            kept += len(want)
    assert kept > 0 or not nms


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", GRAPHS)
def test_world_graph_matches_reference(tag, precision):
    """ONE engine over both shapes: y and the raw maps of every level under the bounds, and NMS at the fixture's conf: on the fixture's own y
    the device NMS returns the stored rows in every precision, and on the engine's y it is the oracle's NMS of that y bit for bit.  The rows
    kept of the engine's y are NOT compared with the stored rows, in any precision: under the synthetic fill every anchor passes conf 0.25
    and some two dozen of the 504 anchors of the larger shape have their two best classes within 1e-3 of each other, so two predictions
    that agree to 1e-3 legitimately keep different rows (the oracle's NMS of a stored y moved by 1e-5 kept 42 rows where it had kept 41)."""
    z, meta = fixture(tag)
    eng = _engine(tag, precision)
    assert eng.nc == NC and eng.text_nc == NC and eng.meta["world"] and eng.task == "detect"
    _compare(eng, z, meta, precision, NC, "y%d", "raw%d_%d", tag)
    eng.close()


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_world_graph_under_five_rows(precision):
    """Scale n scored against the 5-row text (what set_classes leaves behind): cfg["nc"] = 12 still sizes c3, the outputs have 5 classes."""
    tag = GRAPHS[0]
    z, meta = fixture(tag)
    eng = _engine(tag, precision, txt=_texts()[1])
    assert eng.nc == NC2 and eng.names == {i: str(i) for i in range(NC2)}
    _compare(eng, z, meta, precision, NC2, "y5_%d", "raw5_%d_%d", tag + " 5 rows", nms=False)
    eng.close()


@gpu
@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_text_replacement(precision):
    """load_weights(sd, txt_feats=t2) with the same row count returns the bits of a fresh engine built with t2, which differ from those under
    t1; another row count raises ValueError and leaves the engine as it was."""
    tag = GRAPHS[0]
    meta = fixture(tag)[1]
    t1 = _texts()[0]
    t2 = torch.nn.functional.normalize(torch.randn(NC, E, generator=torch.Generator().manual_seed(9)), dim=-1)  # (nc, E): the other accepted shape
    eng = _engine(tag, precision)
    under1 = outputs(eng, meta, _hw(precision))
    eng.load_weights(_sd_of(tag), txt_feats=t2)
    under2 = outputs(eng, meta, _hw(precision))
    fresh = _engine(tag, precision, txt=t2)
    want2 = outputs(fresh, meta, _hw(precision))
    fresh.close()
    for a, b, c in zip(under2, want2, under1):
        assert all(torch.equal(u, v) for u, v in zip(a, b)) and not torch.equal(a[0], c[0])
    with pytest.raises(ValueError, match="has 5 rows"):
        eng.load_weights(_sd_of(tag), txt_feats=_texts()[1])
    again = outputs(eng, meta, _hw(precision))
    assert all(torch.equal(u, v) for a, b in zip(again, under2) for u, v in zip(a, b))
    eng.load_weights(dict(_sd_of(tag), txt_feats=t1))  # the reserved key of the state dict
    back = outputs(eng, meta, _hw(precision))
    assert all(torch.equal(u, v) for a, b in zip(back, under1) for u, v in zip(a, b))
    eng.load_weights(_sd_of(tag))  # a model's state dict holds no text: the text in use stays
    assert torch.equal(eng.txt_feats, t1) and all(torch.equal(u, v) for a, b in zip(outputs(eng, meta, _hw(precision)), under1) for u, v in zip(a, b))
    eng.load_weights(_sd_of(tag), txt_feats=t2)
    eng.load_weights({k: v * (0.5 if k == "model.16.conv.weight" else 1.0) for k, v in _sd_of(tag).items()})  # new weights, t2 kept
    moved = outputs(eng, meta, _hw(precision))
    assert torch.equal(eng.txt_feats, t2) and not torch.equal(moved[0][0], under2[0][0]) and not torch.equal(moved[0][0], under1[0][0])
    eng.close()
    from bs_yolo_amd.engine import YoloEngine
    with pytest.raises(ValueError, match="needs its text features"):
        YoloEngine(cfg_of(meta), _sd_of(tag), precision=precision)
    with pytest.raises(NotImplementedError, match="per-image text features"):
        YoloEngine(cfg_of(meta), _sd_of(tag), precision=precision, txt_feats=t1.repeat(2, 1, 1))
    with pytest.raises(ValueError, match="rows of E = 512"):
        YoloEngine(cfg_of(meta), _sd_of(tag), precision=precision, txt_feats=t1[..., :256])


class _Seq(torch.nn.Module):
    def __getitem__(self, i):
        return getattr(self, str(i) if i >= 0 else str(max(int(k) for k in self._modules if k.isdigit())))


class WorldModel(RefModel):
    """RefModel for the reference's WorldModel of yolov8-worldv2.yaml (tests/test_yolov6.py's V6Model): `txt_feats` as a plain attribute (not
    in the state dict), an `act` on every Conv module (nn.Identity() on the C2fAttn blocks' proj_conv, nn.SiLU() elsewhere), layers
    indexable as model.model[i], a head with `nc`, and an original forward that says which keywords each call got."""

    def __init__(self, cfg, sd, txt):
        super().__init__(cfg, sd, module_cls=_Seq)
        for name, mod in list(self.named_modules()):
            if hasattr(mod, "conv") and hasattr(mod, "bn"):
                mod.act = torch.nn.Identity() if name.endswith("attn.proj_conv") else torch.nn.SiLU()
        self.txt_feats = txt.clone()
        self.model[-1].nc = txt.shape[-2]
        self.calls = []
        self.eval()

    def forward(self, x, *args, **kwargs):
        self.calls.append(sorted(kwargs))
        return "original"


@gpu
def test_accelerate_a_world_model():
    from bs_yolo_amd import plugin
    tag = GRAPHS[0]
    z, meta = fixture(tag)
    t1, t2 = _texts()
    m = WorldModel(cfg_of(meta), _sd_of(tag), t1).to(DEV)
    assert "txt_feats" not in m.state_dict() and m.model[-1].nc == NC
    plugin.accelerate(m)
    st = m._bsy_state
    assert st["support"] == {"fp16": True, "fp32": True}
    x = x_of(meta, 1)
    b, h, w = meta["shapes"][1]
    levels = [(h // int(s), w // int(s)) for s in meta["stride"]]
    lvl, A = level_of_anchor(levels), sum(lh * lw for lh, lw in levels)
    out = m(x.to(DEV))  # fp32 input: the fp32x engine
    assert isinstance(out, tuple) and len(out) == 2 and isinstance(out[1], list) and len(out[1]) == 3 and not m.calls and st["fp32_calls"] == 1
    y, raws = out
    assert tuple(y.shape) == (b, 4 + NC, A) and [tuple(r.shape) for r in raws] == [(b, 64 + NC, lh, lw) for lh, lw in levels]
    check_y(y.cpu().numpy(), z["y1"], meta["stride"], lvl, max(h, w), "fp32x", "accelerate", NC, Y_BOUNDS)
    y16, raws16 = m(x.half().to(DEV))
    assert st["engine_calls"] == 1 and not m.calls and st["engine"].nc == NC
    check_y(y16.float().cpu().numpy(), z["y1"], meta["stride"], lvl, max(h, w), "fp16", "accelerate", NC, Y_BOUNDS)
    for l, r in enumerate(raws16):
        check_raw(r.float().cpu().numpy(), z[f"raw1_{l}"], "fp16", f"accelerate raw {l}", RAW_BOUNDS)
    # a call with its own text goes to the original forward; so does augment (the class is not DetectionModel)
    n_fb = st["fallbacks"]
    assert m(x.half().to(DEV), txt_feats=t2.to(DEV)) == "original" and m.calls == [["txt_feats"]] and st["fallbacks"] == n_fb + 1
    assert m(x.half().to(DEV), augment=True) == "original" and st["fallbacks"] == n_fb + 2
    assert m(x.half().to(DEV), txt_feats=None)[0].shape == y16.shape and len(m.calls) == 2  # None: the model's own text, the engine's
    # set_classes: a new tensor with 5 rows and head.nc = 5 -> one rebuild, a new plan
    n = st["rebuilds"]
    m.txt_feats, m.model[-1].nc = t2.clone(), NC2
    y5, raws5 = m(x.half().to(DEV))
    assert st["rebuilds"] == n + 1 and tuple(y5.shape) == (b, 4 + NC2, A) and [r.shape[1] for r in raws5] == [64 + NC2] * 3 and st["engine"].nc == NC2
    check_y(y5.float().cpu().numpy(), z["y5_1"], meta["stride"], lvl, max(h, w), "fp16", "accelerate 5 rows", NC2, Y_BOUNDS)
    m(x.half().to(DEV))
    assert st["rebuilds"] == n + 1  # nothing changed: no rebuild
    # an in-place edit of the text rebuilds too
    with torch.no_grad():
        m.txt_feats[0, 0] = m.txt_feats[0, 1]
    y5b, _ = m(x.half().to(DEV))
    assert st["rebuilds"] == n + 2 and not torch.equal(y5b, y5) and torch.equal(y5b[:, 4], y5b[:, 5])
    assert len(m.calls) == 2
    plugin.restore(m)
    assert m(x.to(DEV)) == "original"
