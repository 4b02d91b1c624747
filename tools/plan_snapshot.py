"""Digests of everything a Plan hands to the device and to the weight packer, for a fixed matrix of graphs, precisions and options:
the regression fixture of host-side refactors of bs_yolo_amd/plan.py (tests/test_host_logic.py, tests/golden/plan_snapshots.json).

    python tools/plan_snapshot.py                   print "<case> <ops> <digest>" per case and compare with the fixture
    python tools/plan_snapshot.py --dump DIR        also write every case's plain-text form to DIR/<case>.txt (diff two commits' DIRs);
                                                    there every case packs, in its precision's layout: see "host:" below
    python tools/plan_snapshot.py --write           rewrite the fixture -- ONLY at a commit whose plans are known to be right

A snapshot is the sha256 of the text that --dump writes: the serialised op array (after packing synthetic weights, or with running
record offsets where a case is not packed), buffer sizes, flops, meta, layer outputs, weight records, the host-side op fields
(name, mfma_flops, cout, weight keys), both arena layouts and the autotuner's conv signatures.  Lines that begin with "host:" are
written but not hashed: the packed blob's sha256 and ELA's exact coefficients come out of torch's CPU kernels (randn, sigmoid), whose
last bits differ from one CPU to the next, so they compare between two commits on ONE machine only; the digest holds the blob's
length, every record's offsets and the coefficients to four decimals.  A case whose digest is taken with running offsets gets its
packed blob's length, sha256 and coefficients as "host:" lines in a dump (packed from a second plan, so the hashed text stays as it is):
two commits' dumps then compare the weight bytes of every case, fp32 and fp32x layouts included.  Needs no GPU."""
import dataclasses
import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from bs_yolo_amd import lib as L  # noqa: E402
from bs_yolo_amd.graphs import stock_cfg  # noqa: E402
from bs_yolo_amd.plan import Plan  # noqa: E402
from bs_yolo_amd.weights import pack_plan_weights, synth_state_dict  # noqa: E402

FIXTURE = ROOT / "tests" / "golden" / "plan_snapshots.json"
SWITCH_ENV = {"fuse_stem": "BSY_FUSE_STEM", "fuse_bneck": "BSY_FUSE_BNECK", "fuse_head": "BSY_FUSE_HEAD", "fuse_dwpw": "BSY_FUSE_DWPW",
              "merge_c3k": "BSY_MERGE_C3K", "fuse_msca": "BSY_FUSE_MSCA", "fuse_tail": "BSY_FUSE_TAIL", "fuse_pmsfa": "BSY_FUSE_PMSFA",
              "fuse_attn_pe": "BSY_FUSE_ATTN_PE"}
PLAN_ENV = tuple(SWITCH_ENV.values()) + ("BSY_FUSE_BOXTAIL", "BSY_FUSE_GHOST", "BSY_LANES", "BSY_FUSE_FIRST_POOL")  # what a Plan reads from the environment
ALL_OFF = {k: False for k in SWITCH_ENV}
OPTIONS = {"default": {}, "unfused": ALL_OFF, "latency_lanes": dict(latency=True, lanes=True)}
# (family, scale, task, (B, H, W))
MATRIX = [("yolo11", "n", "detect"), ("yolo11", "s", "detect"), ("yolo11", "m", "segment"), ("yolo11", "s", "obb"), ("yolov8", "s", "detect"),
          ("bsyolo11", "s", "detect"), ("yolov5", "s", "detect"), ("yolov8-p2", "s", "detect"), ("yolov9", "t", "detect"),
          ("yolov9", "m", "detect"), ("yolov9", "c", "segment")]
MATRIX = [g + ((2, 64, 96),) for g in MATRIX] + [("yolov8-p6", "s", "detect", (2, 128, 192)), ("yolov5-p6", "s", "detect", (2, 128, 192))]
# The families behind YOLOv9 and the pose / classify plans: (case name, () -> graph, (B, H, W), Plan keywords in every option)
_S, _L = (2, 64, 96), (2, 128, 192)
MATRIX2 = [
    ("yolo11-n-pose", lambda: stock_cfg("yolo11", "n", 1, "pose", kpt_shape=(17, 3)), _S, {}),
    ("yolov8-p6-s-pose", lambda: stock_cfg("yolov8-p6", "s", 1, "pose", kpt_shape=(17, 3)), _L, {}),
    ("yolo11-n-classify", lambda: stock_cfg("yolo11", "n", 1000, "classify"), _S, {}),
    ("yolov8-s-classify", lambda: stock_cfg("yolov8", "s", 10, "classify"), _S, {}),
    ("yolov10-n-detect", lambda: stock_cfg("yolov10", "n"), _S, {}),
    ("yolov10-b-detect", lambda: stock_cfg("yolov10", "b"), _S, {}),
    ("yolov10-s-one2many-k50", lambda: stock_cfg("yolov10", "s"), _S, dict(one2many=True, max_det=50)),
    ("yolov8-ghost-s-detect", lambda: stock_cfg("yolov8-ghost", "s"), _S, {}),
    ("yolov8-ghost-p2-n-detect", lambda: stock_cfg("yolov8-ghost-p2", "n"), _S, {}),  # its C3Ghost: ghostconv on padded pieces
    ("yolov8-ghost-p6-s-detect", lambda: stock_cfg("yolov8-ghost-p6", "s"), _L, {}),
    ("yolov3-detect", lambda: stock_cfg("yolov3", None), _S, {}),
    ("yolov3-spp-detect", lambda: stock_cfg("yolov3-spp", None), _S, {}),
    ("yolov3-tiny-detect", lambda: stock_cfg("yolov3-tiny", None), _S, {}),
    ("yolov6-n-detect", lambda: stock_cfg("yolov6", "n"), _S, {}),
    ("yolov6-m-sppf-relu", lambda: stock_cfg("yolov6", "m"), _S, dict(sppf_act="relu")),
]


def clear_env():
    for k in PLAN_ENV:
        os.environ.pop(k, None)


def _width(family, width, scale="n"):
    return dict(stock_cfg(family, scale), scale="t", scales={"t": [0.5, width, 1024]})


def cases():
    """[(case id, () -> Plan, pack)].  pack: synthetic weights are packed and the blob's digest is part of the snapshot; the other cases
    serialise with running record offsets (the op array then still says which record every op reads)."""
    out = []
    for fam, scale, task, shape in MATRIX:
        for prec in ("fp16", "fp32", "fp32x"):
            for oname, kw in OPTIONS.items():
                out.append((f"{fam}-{scale}-{task}/{prec}/{oname}",
                            lambda fam=fam, scale=scale, task=task, shape=shape, prec=prec, kw=kw: Plan(stock_cfg(fam, scale, 80, task), *shape, precision=prec, **kw),
                            oname == "default" and prec == "fp16"))
    for cname, graph, shape, fixed in MATRIX2:
        for prec in ("fp16", "fp32", "fp32x"):
            for oname, kw in OPTIONS.items():
                out.append((f"{cname}/{prec}/{oname}",
                            lambda graph=graph, shape=shape, prec=prec, kw=dict(fixed, **kw): Plan(graph(), *shape, precision=prec, **kw),
                            oname == "default" and prec == "fp16"))
    s11 =lambda: stock_cfg("yolo11", "s")  # noqa: E731
    out += [
        ("extra/yolov8-p6-s-segment", lambda: Plan(stock_cfg("yolov8-p6", "s", 80, "segment"), 2, 128, 192), True),
        ("extra/yolo11-x", lambda: Plan(stock_cfg("yolo11", "x"), 2, 64, 64), True),
        ("extra/yolov8-l-segment-640", lambda: Plan(stock_cfg("yolov8", "l", 80, "segment"), 1, 640, 640), True),
        ("extra/yolo11-s-16x640", lambda: Plan(s11(), 16, 640, 640), True),
        ("extra/yolo11-s-16x640-lanes-off", lambda: Plan(s11(), 16, 640, 640, lanes=False), False),
        ("extra/yolo11-s-16x640-lanes-on", lambda: Plan(s11(), 16, 640, 640, lanes=True), False),
        ("extra/yolo11-s-8x640-latency", lambda: Plan(s11(), 8, 640, 640, latency=True), True),
        ("extra/yolo11-n-nc100", lambda: Plan(stock_cfg("yolo11", "n", 100), 2, 64, 96), True),
        ("extra/yolov9-c-repvgg", lambda: Plan(stock_cfg("yolov9", "c"), 2, 64, 96, repconv="repvgg"), True),
        ("extra/yolo11-s-u8-f32", lambda: Plan(s11(), 2, 64, 96, in_dtype=L.BSY_U8, out_dtype=L.BSY_F32), True),
        ("width/yolo11-0.1875", lambda: Plan(_width("yolo11", 0.1875), 2, 96, 64), True),
        ("width/yolov8-0.3125", lambda: Plan(_width("yolov8", 0.3125), 2, 96, 64), True),
        ("width/yolov5-0.3125", lambda: Plan(_width("yolov5", 0.3125), 2, 96, 64), True),
        ("width/bsyolo11-0.375", lambda: Plan(_width("bsyolo11", 0.375), 2, 96, 64), True),
        ("width/bsyolo11-0.1875-fp32", lambda: Plan(_width("bsyolo11", 0.1875), 2, 96, 64, precision="fp32"), True),
        ("width/yolo11-0.3125-fp32", lambda: Plan(_width("yolo11", 0.3125), 2, 96, 64, precision="fp32"), True),
        # CIB on padded pieces, without and (the b graph) with lk
        ("width/yolov10-n-0.1875", lambda: Plan(_width("yolov10", 0.1875), 2, 96, 64), True),
        ("width/yolov10-n-0.375", lambda: Plan(_width("yolov10", 0.375), 2, 96, 64), True),
        ("width/yolov10-b-0.375", lambda: Plan(_width("yolov10", 0.375, "b"), 2, 96, 64), True),
    ]
    return out


def _t(t):
    if t is None:
        return "-"
    if isinstance(t, (list, tuple)):
        return "[" + " ".join(_t(u) for u in t) + "]"
    return f"({t.buf},{t.ld},{t.coff},{t.C},{t.H},{t.W},{int(t.up)},{int(t.f32)},{t.cmap})"


def _packed(plan):
    """Packs synthetic weights into `plan` -> (blob length, the "host:" lines of the blob's sha256 and ELA's exact coefficients)."""
    blob = pack_plan_weights(plan, synth_state_dict(plan))
    return len(blob), [f"host: blob {hashlib.sha256(blob).hexdigest()}"] + [f"host: coef {k} {r.coef}" for k, r in plan.wrecs.items() if r.kind == "ela"]


def snapshot_text(plan, pack, host_plan=None):
    """The plain-text form of one plan (see the module docstring).  host_plan: a second plan of an unpacked case, packed for its
    "host:" lines."""
    lines = []
    if pack:
        n, host = _packed(plan)
        lines += [f"blob {n} bytes"] + host
        for r in plan.wrecs.values():
            r.coef = tuple(round(c, 4) for c in r.coef)
    else:
        if host_plan is not None:
            n, host = _packed(host_plan)
            lines += [f"host: blob {n} bytes"] + host
        for i, r in enumerate(plan.wrecs.values()):
            r.w_off, r.b_off = 512 * i, 512 * i + 256
    raw = bytes(plan.c_ops())
    n = len(raw) // max(len(plan.ops), 1)
    lines.append(f"ops {len(plan.ops)} bufs {plan.buf_bytes} flops {plan.flops}")
    lines.append(f"meta {sorted(plan.meta.items())}")
    lines += [f"layer {i} {_t(t)}" for i, t in enumerate(plan.layer_out)]
    lines += [f"wrec {k} {dataclasses.astuple(r)}" for k, r in plan.wrecs.items()]
    for i, o in enumerate(plan.ops):
        lines.append(f"op {i} {o['name']} kind {o['kind']} mfma_flops {o.get('mfma_flops')} cout {o.get('cout')} wkey {o.get('wkey')} "
                     f"wkey2 {o.get('wkey2')} wkeys {o.get('wkeys')} sig {plan.conv_signature(o)}")
        lines.append(f"   {raw[i * n:(i + 1) * n].hex()}")
    lines.append(f"arena reuse {plan.assign_offsets(True)}")
    lines.append(f"arena plain {plan.assign_offsets(False)}")
    return "\n".join(lines) + "\n"


def snapshot(build, pack, host=False):
    plan = build()
    text = snapshot_text(plan, pack, build() if host and not pack else None)
    hashed = "".join(ln for ln in text.splitlines(True) if not ln.startswith("host:"))
    return {"digest": hashlib.sha256(hashed.encode()).hexdigest(), "ops": len(plan.ops)}, text


def main(argv):
    clear_env()
    dump = Path(argv[argv.index("--dump") + 1]) if "--dump" in argv else None
    if dump:
        dump.mkdir(parents=True, exist_ok=True)
    have = json.loads(FIXTURE.read_text()) if FIXTURE.exists() else {}
    got, bad = {}, []
    for cid, build, pack in cases():
        got[cid], text = snapshot(build, pack, host=dump is not None)
        if dump:
            (dump / (cid.replace("/", "__") + ".txt")).write_text(text)
        if have and have.get(cid) != got[cid]:
            bad.append(cid)
        print(cid, got[cid]["ops"], got[cid]["digest"], "DIFFERS" if cid in bad else "")
    if "--write" in argv:
        FIXTURE.write_text(json.dumps(got, indent=0, sort_keys=True) + "\n")
        print("wrote", FIXTURE)
    elif bad:
        print(f"{len(bad)} of {len(got)} cases differ from {FIXTURE}")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
