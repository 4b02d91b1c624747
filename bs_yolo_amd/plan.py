"""Host-side graph flattening: model description -> flat list of device ops (include/bsyolo.h `bsy_op`).

Mirrors what the reference does at run time in Python:
  * nn/tasks.py:940-1105 parse_model  -- channel scaling ``make_divisible(min(c2, max_ch) * width, 8)`` (:1016),
    repeat scaling ``max(round(n * depth), 1)`` (:972), ``c3k=True`` for m/l/x (:1046-1049), ``legacy`` Detect head
    for graphs without C3k2 (:1048, head.py:44-56);
  * nn/tasks.py:138-165 _predict_once -- the ``f`` / save routing between top-level layers;
  * the forward of every module on the path (conv.py:133-151; block.py:3114-3149, 3295-3334, 3405-3419, 3796-3815,
    4235-4288, 4348-4383, 4429-4468; head.py:64-131).
Instead of executing modules, every forward is expanded into device ops over NHWC buffers:
  chunk/split/cat -> channel-slice views of one buffer; nn.Upsample -> `up` flag on the consumer's source;
  Concat -> two-source conv; shortcut adds -> conv epilogue residual.

The model description is the reference's own yaml dict schema (``model.yaml`` of a live reference model, or the
stock tables in graphs.py), so a reference model drops in without translation.
"""
from __future__ import annotations

import functools
import math
import os
from collections import OrderedDict, namedtuple
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

from . import lib as L


def make_divisible(x, d):  # utils/ops.py:130-143
    return math.ceil(x / d) * d


@dataclass
class T:
    """A logical NHWC activation: channel slice [coff, coff+C) of buffer `buf` (row stride `ld`), H x W pixels.
    up=True: stored at (H/2, W/2), read through nearest x2 (virtual nn.Upsample)."""
    buf: int
    ld: int
    coff: int
    C: int
    H: int
    W: int
    up: bool = False
    f32: bool = False
    # Zero-padded pieces (round 4; the fp16 path reads 8-channel pieces, so a C2f / C3k2 whose chunk width is 12 or 20 channels carries every
    # chunk on the next multiple of 8): cmap[j] = which REAL channel of this tensor the stored channel j is, or -1 for a padding channel
    # that is always zero (zero weight rows and bias where it is written, SiLU(0) = 0; zero weight columns where it is read).  None = all real.
    cmap: Optional[Tuple[int, ...]] = None

    def slice(self, c0: int, c: int) -> "T":
        assert 0 <= c0 and c0 + c <= self.C
        cm = None
        if self.cmap is not None:
            before = sum(1 for v in self.cmap[:c0] if v >= 0)
            cm = tuple(v - before if v >= 0 else -1 for v in self.cmap[c0:c0 + c])
            if all(v >= 0 for v in cm):
                cm = None
        return T(self.buf, self.ld, self.coff + c0, c, self.H, self.W, self.up, self.f32, cm)

    @property
    def real(self) -> int:
        """Channels that carry data (== C unless the tensor has padding pieces)."""
        return self.C if self.cmap is None else sum(1 for v in self.cmap if v >= 0)

    def padded(self, pieces: Sequence[Tuple[int, int]]) -> "T":
        """This tensor seen as consecutive (stored width, real width) pieces, each zero-padded at its end."""
        cm, base = [], 0
        for width, real in pieces:
            cm += [base + i if i < real else -1 for i in range(width)]
            base += real
        assert len(cm) == self.C
        return T(self.buf, self.ld, self.coff, self.C, self.H, self.W, self.up, self.f32, tuple(cm))

    def view(self):
        return (self.buf, self.ld, self.coff, self.C)


@dataclass
class WRec:
    """How to pack one op's parameters into the weight blob (weights.py)."""
    name: str          # state_dict prefix, e.g. "model.2.m.0.cv1"  (Conv: .conv.weight + .bn.*; plain: .weight/.bias)
    kind: str          # conv | conv2 (name + post stacked along cout) | plain | dw | first | deconv
    cout: int
    cin: int
    k: int
    perm: Optional[List[int]] = None   # output-channel permutation (qkv)
    tap: Optional[Tuple[int, int]] = None  # deconv: (dy, dx)
    kw: Optional[int] = None           # dwg: kernel width when != k (strip convs)
    post: Optional[str] = None         # dwg: name of a depthwise 1x1 conv folded in after this one (MSCA dilconv)
    coef: Tuple[float, float, float] = (0.0, 0.0, 0.0)  # ela: sigmoid(ch_weight / sp_weight / res_weight), set when packed
    real_cout: int = 0                 # the module's own output / input channels where the op runs on a width padded to a multiple of 8
    real_cin: int = 0                  # (Detect's class branch with nc-dependent widths, head.py:39): zero weights in the padding; 0 = as cout / cin
    rows: Optional[List[int]] = None   # op output channel i takes the module's output channel rows[i] (-1: a zero channel, weights and bias 0);
    cols: Optional[List[int]] = None   # op input channel j is the module's input channel cols[j] (-1: zero weights) -- PMSFA on padded pieces
    w_off: int = -1
    b_off: int = -1
    # maxsig / world_cls: the width E of the text features the record folds in (state-dict key "txt_feats").  A plain attribute set by
    # Plan._wrec, not a dataclass field: a record's field tuple is part of the plan snapshots (tools/plan_snapshot.py)
    embed = 0


def qkv_perm(nh: int, kd: int, hd: int) -> List[int]:
    """Attention.qkv's output rows are emitted per head as [q(kd) k(kd) v(hd)] by the reference (block.py:4274-4276); the kernels
    want [q(all heads) | k(all heads) | v(all heads)], so that v is one channel slice and heads are contiguous: row i of that order
    is the module's row qkv_perm(...)[i]."""
    per = 2 * kd + hd
    return [h * per + off + i for off, n in ((0, kd), (kd, kd), (2 * kd, hd)) for h in range(nh) for i in range(n)]


# Fusion switch -> the environment variable that decides it where the caller passes None. Every switch defaults to on, and the
# fp32-storage modes clear them all.  A new switch is one line here: Plan and YoloEngine take it as a keyword from this table.
SWITCHES = {
    "fuse_stem": "BSY_FUSE_STEM",        # layers 0 + 1 as one launch (csrc/stem_fused.hip); off: two launches
    "fuse_bneck": "BSY_FUSE_BNECK",      # Bottleneck with the hidden map in LDS (csrc/bneck_fused.hip)
    "fuse_head": "BSY_FUSE_HEAD",        # Detect's last convs decode in their epilogue; off: f32 logit maps + the decode launch
    "fuse_dwpw": "BSY_FUSE_DWPW",        # DWConv 3x3 + Conv 1x1 of the class branch as one launch (csrc/dwpw_fused.hip)
    "merge_c3k": "BSY_MERGE_C3K",        # C3k's cv1 and cv2 as one conv of twice the width
    "fuse_msca": "BSY_FUSE_MSCA",        # MSCAAttention's nine depthwise convs and four means as one launch
    "fuse_tail": "BSY_FUSE_TAIL",        # a whole C3k2 block as one launch (csrc/c3k2_fused.hip)
    "fuse_pmsfa": "BSY_FUSE_PMSFA",      # PMSFA's depthwise 5x5 -> depthwise 7x7 -> 1x1 + shortcut as one launch (round 4, csrc/pmsfa_fused.hip)
    "fuse_attn_pe": "BSY_FUSE_ATTN_PE",  # Attention.pe (depthwise 3x3 on v + the attention output) in the attention kernel's epilogue
}

@functools.lru_cache(maxsize=256)
def kernel_takes(kernel: str, *shape: int) -> bool:
    """Whether a fused kernel runs a shape: the library's own answer, bsy_<kernel>_supported(*shape) of include/bsyolo.h (the planner
    keeps no list of its own).  Remembered: every new input shape builds a plan, and each asks the same few questions."""
    return getattr(L.lib, f"bsy_{kernel}_supported")(*shape) == 1


# Every field an op dict may carry besides kind / name / lane.  The scalars that c_ops() copies into the bsy_op member of the same name,
# with what an op that lacks them serialises (a new scalar field is one entry here); the members c_ops() fills by hand -- sizes, views,
# per-level view lists and numbers; and what only the host reads (the weight record keys, and `cout` / `mfma_flops` for the autotuner's
# signature and the benchmark's per-family sums).  Plan._emit refuses anything else: a misspelt key would serialise as its default.
SCALAR_FIELDS = (("ksize", 0), ("stride", 0), ("pad", 0), ("act", 0), ("out_f32", 0), ("dst_scale", 1), ("dst_dy", 0), ("dst_dx", 0),
                 ("mid_c", 0), ("heads", 0), ("key_dim", 0), ("head_dim", 0), ("scale", 0.0), ("nl", 0), ("nc", 0), ("nm", 0), ("ne", 0),
                 ("A", 0), ("nk", 0), ("kdim", 0), ("in_dtype", 0), ("out_dtype", 0), ("level", 0), ("join", 0), ("ksplit", 0))
VIEW_FIELDS, LIST_FIELDS, LEVEL_FIELDS = ("src0", "src1", "dst", "res"), ("box", "cls", "msk"), (("lvl_h", 0), ("lvl_w", 0), ("lvl_stride", 0.0))
OP_FIELDS = frozenset(("H", "W", "OH", "OW") + VIEW_FIELDS + LIST_FIELDS + tuple(f for f, _ in LEVEL_FIELDS + SCALAR_FIELDS)
                      + ("wkey", "wkey2", "wkeys", "cout", "mfma_flops"))
# kinds that may run on a side lane (csrc/engine.hip bsy_plan_run forks and joins around them)
LANE_KINDS = (L.OP_CONV, L.OP_DWCONV, L.OP_BNECK, L.OP_DWCONV_G, L.OP_DWPW, L.OP_C3K2)
Output = namedtuple("Output", "name slot shape dtype raw_only")  # one external output of a plan (Plan._ext, Plan.outputs)


@dataclass
class _ZeroPadded:
    """What an accepted nn.ZeroPad2d [[0, 1, 0, 1]] layer hands to the nn.MaxPool2d [2, 1, 0] behind it: its input, unpadded."""
    src: T

    def gate(self, i: int, m: str):
        if m != "nn.MaxPool2d":
            raise NotImplementedError(f"model.{i - 1}: nn.ZeroPad2d is accelerated only in front of nn.MaxPool2d [2, 1, 0] (model.{i} is {m})")


@dataclass
class _Slices:
    """What a CBLinear layer (block.py:3740-3757) hands on: the channel groups of its one conv's output, as views of that buffer.  Only a
    CBFuse may read it (Plan._build refuses every other consumer by name)."""
    parts: List[T]
    layer: int


class _Layer:
    """What the graph walk hands to a layer's lowering (Plan.LOWERINGS): the layer's index, its name "model.i", its module, its input x
    (`f` resolved: a T, a list of T behind a Concat, a _ZeroPadded, a _Slices or a list that holds some in front of a CBFuse, or None for
    the image), its arguments with "nc" resolved, its repeat
    count depth-scaled, args[0] width-scaled where the table says the module's is (else None), and whether it is the graph's last.
    ONE record per walk, refilled for every layer (a fresh one each was 5 % of plan construction): a lowering reads it and keeps none."""
    __slots__ = ("i", "name", "m", "x", "args", "n", "c2", "last")

    def arg(self, j: int, default):
        return self.args[j] if len(self.args) > j else default


class Plan:
    """Flat op list + workspace buffer table for one (B, H, W)."""

    EXT_IMG, EXT_Y, EXT_RAW0 = 0, 1, 2  # external slots (the one numbering; a plan's own are in `outputs`): image, prediction, raw level maps (2, 3, 4)
    EXT_PROTO = EXT_KPT = 5  # a segment plan's proto, or a pose plan's raw keypoint logits (B, nk, A): a plan has one or the other
    EXT_RAW3 = 6  # the fourth level's raw map (P2 / P6 heads): behind the proto slot, so that slots 0-5 stay what they were
    EXT_LOGITS, EXT_TOPK_IDX, EXT_TOPK_VAL = 2, 3, 4  # a classify plan's slots behind image and y: x (the logits), the top-k rows
    # An end2end (v10Detect) plan: the pre-top-k tensor `pre` takes y's slot and the one2one raw maps `o2o{l}` the raw slots; behind
    # every slot an earlier plan uses come the top-k rows and the one2many raw maps `o2m{l}` (levels 0 .. 3 at 8 .. 11)
    EXT_ROWS, EXT_O2M0 = 7, 8

    @classmethod
    def ext_raw(cls, level: int) -> int:
        """External slot of level `level`'s raw map."""
        assert 0 <= level < L.BSY_MAX_LEVELS
        return cls.EXT_RAW0 + level if level < 3 else cls.EXT_RAW3 + level - 3

    def _ext(self, name: str, slot: int, C: int, tail: Tuple[int, ...] = (), dtype: str = "io", raw_only: bool = False) -> T:
        """The view of external slot `slot`, C channels wide.  Every slot but the image is an output and enters `outputs` by name: shape (B, C) + tail,
        dtype ("io": the plan's out_dtype), raw_only (only a caller that wants the raw outputs has it); a name met again (y, at every fused level) says the same."""
        if slot != self.EXT_IMG:
            out = Output(name, slot, (self.B, C) + tuple(tail), dtype, raw_only)
            assert self.outputs.get(name, out) == out, f"external output {out} after {self.outputs[name]}"
            self.outputs[name] = out
        return T(L.BSY_EXT_BASE + slot, 0, 0, C, *(tail if slot == self.EXT_IMG else (0, 0)))  # (the image's view alone carries its size)

    def _raw(self, level: int, nc: int, x: T) -> T:  # the view of level `level`'s raw map (B, no, h, w), `x` being any map of that level
        if self._e2e == "o2m":
            return self._ext(f"o2m{level}", self.EXT_O2M0 + level, 64 + nc, (x.H, x.W), raw_only=True)
        return self._ext(f"o2o{level}" if self._e2e else f"raw{level}", self.ext_raw(level), 64 + nc, (x.H, x.W), raw_only=True)

    def _y(self, rows: int, A: int) -> T:  # the prediction tensor (B, rows, A): `y`, or an end2end head's pre-top-k tensor `pre`
        return self._ext("pre" if self._e2e else "y", self.EXT_Y, rows, (A,))

    def __init__(self, cfg: dict, B: int, H: int, W: int, in_dtype: int = L.BSY_F16, out_dtype: int = L.BSY_F16, precision: str = "fp16",
                 lanes: Optional[bool] = None, latency: bool = False, repconv: str = "refconv", max_det: int = 300, one2many: bool = False,
                 sppf_act: str = "silu", text_nc: Optional[int] = None, **switches: Optional[bool]):
        """switches: the keys of SWITCHES; None (or absent) = what the switch's environment variable says, on where it is unset.
        text_nc: read by a YOLO-World graph (a WorldDetect head) alone -- the number of classes SCORED, the rows of the text features; None
        = cfg["nc"].  It sizes the guide records of the C2fAttn blocks, the folded class convs, meta["nc"] and the A x (4 + nc) prediction;
        cfg["nc"] keeps sizing the head's hidden width c3 as the constructor did (head.py:313), whatever set_classes chose later.
        max_det, one2many: read by a v10Detect head alone -- the rows its top-k keeps, and whether the one2many branches (cv2 / cv3, raw
        maps only, which a caller who wants the rows alone must not pay for) are part of the plan."""
        if not set(switches) <= set(SWITCHES):
            raise TypeError(f"Plan() got an unexpected keyword argument {sorted(set(switches) - set(SWITCHES))[0]!r}")
        self.cfg, self.B, self.H, self.W = cfg, B, H, W
        # What RepBottleneck.cv1 (YOLOv9's RepCSP, block.py:3634-3641) is in the model at hand: "refconv", the fork's own RepConv
        # (block.py:793-816: one bare 3x3 conv whose kernel is weight + convmap(weight); no BN, no bias, no activation) -- what every
        # yaml-built model holds --, or "repvgg", upstream's (conv.py:296-397: SiLU(conv3x3 + conv1x1), each with BN; folds into one
        # biased 3x3) -- what an upstream-pickled checkpoint unpickles.  plugin.accelerate tells them apart by the state-dict keys.
        if repconv not in ("refconv", "repvgg"):
            raise ValueError(f"repconv must be 'refconv' or 'repvgg', not {repconv!r}")
        self.repconv = repconv
        # What SPPF's cv1 / cv2 apply in a graph whose yaml says `activation: nn.ReLU()` (YOLOv6); read nowhere else.  "silu" is what every
        # yaml-built model of this fork holds: nn/modules/block.py:13 does `from ..Addmodules import *`, which shadows `Conv` for every
        # class of block.py, and parse_model sets `default_act` on nn.modules.conv.Conv alone (tasks.py:956-957) -- the top-level Convs
        # and the Detect head turn ReLU, SPPF's two Convs stay SiLU.  Upstream has no such shadowing: a model pickled there unpickles
        # with ReLU in SPPF too, which is "relu".  plugin.accelerate and YoloEngine read the form from the live module.
        if sppf_act not in ("silu", "relu"):
            raise ValueError(f"sppf_act must be 'silu' or 'relu', not {sppf_act!r}")
        self.sppf_act = sppf_act
        # the graph's default activation as an id of include/bsyolo.h (1 SiLU, 2 ReLU): what `act=True` means to conv() below
        activation = cfg.get("activation")
        if activation not in (None, "", "nn.SiLU()", "nn.ReLU()"):
            raise NotImplementedError(f"activation {activation!r} (tasks.py:956-957) is not accelerated: nn.SiLU() and nn.ReLU() are")
        self.act_id = L.ACT_RELU if activation == "nn.ReLU()" else L.ACT_SILU
        if not 1 <= int(max_det) <= 4096:
            raise ValueError(f"max_det must be 1 .. 4096 (the top-k sorts its winners in LDS), not {max_det!r}")
        self.max_det, self.one2many = int(max_det), bool(one2many)
        if text_nc is not None and (int(text_nc) != text_nc or text_nc < 1):
            raise ValueError(f"text_nc must be a positive row count, not {text_nc!r}")
        self.text_nc = None if text_nc is None else int(text_nc)
        self._e2e = ""  # which head copy of a v10Detect is being emitted: "" (not an end2end head), "o2o", "o2m"
        # latency mode (round 4; fp16 path): long-K conv layers with few tiles per image run split-K (split_factors below)
        self.latency = bool(latency) and precision == "fp16"
        if precision not in ("fp16", "fp32", "fp32x"):
            raise ValueError(f"precision must be 'fp16', 'fp32' or 'fp32x', not {precision!r}")
        # fp32: the correctness mode (csrc/ref32.hip) -- every buffer f32, no fused kernels, same op list otherwise.
        # fp32x: the same plan; its dense convs multiply on the fp16 matrix pipe with split-f16 operands (csrc/conv32x_mfma.hip)
        self.f32_mode = precision in ("fp32", "fp32x")
        self.split_f16 = precision == "fp32x"
        self.in_dtype, self.out_dtype = in_dtype, out_dtype
        for name, env in SWITCHES.items():
            arg = switches.get(name)
            setattr(self, name, not self.f32_mode and ((os.environ.get(env, "1") != "0") if arg is None else bool(arg)))
        # box-branch tail (cv2.x.1 + cv2.x.2 + DFL in one launch): part of the head fusion; the variable below switches it off alone
        self.fuse_boxtail = self.fuse_head and os.environ.get("BSY_FUSE_BOXTAIL", "1") != "0"
        # GhostConv (1x1 cv1 + depthwise 5x5 cv2 + the GhostBottleneck shortcut) as one launch (csrc/ghost_fused.hip).  Not in SWITCHES: every
        # entry of that table changes one of the graphs the switch test builds, and none of those holds a GhostConv
        self.fuse_ghost = not self.f32_mode and os.environ.get("BSY_FUSE_GHOST", "1") != "0"
        # yolov3-tiny's stride-1 image conv and the MaxPool2d(2, 2, 0) behind it as one launch (BSY_OP_FIRST_POOL, csrc/conv_first.hip).  Not in
        # SWITCHES for the same reason: no graph of the switch test starts with that pair
        self.fuse_first_pool = not self.f32_mode and os.environ.get("BSY_FUSE_FIRST_POOL", "1") != "0"
        self._up_real: Dict[Tuple[int, int, int], T] = {}  # upsampled views a 3x3 conv has had materialised (conv below)
        self.buf_bytes: List[int] = []
        self.ops: List[dict] = []
        self.wrecs: "OrderedDict[str, WRec]" = OrderedDict()
        self.flops = 0  # 2*MAC of every dense/depthwise conv + attention matmuls, whole batch
        self.meta: Dict = {}
        self.outputs: Dict[str, Output] = {}
        self._lane = 0
        self._build()
        if self.latency:
            self._apply_split_k()
        # Side lanes (the Detect branches on their own streams) pay a fork / join event pair each: worth it when the branch kernels
        # are long enough to overlap -- from about 12 images of 640 x 640 (measured: 0.74 vs 0.79 ms at 1 image, 0.94 vs 0.96 at 8,
        # 1.25 vs 1.24 at 16, 1.92 vs 1.87 at 32, 3.3 vs 3.2 at 64).  BSY_LANES=0 / 1 forces one or the other (0: the tests' serial
        # reference schedule).
        # `lanes` (argument): the engine's graph mode asks for them at every size -- in a captured graph fork / join are edges, not events.
        env = os.environ.get("BSY_LANES")
        if env == "0" or (env is None and not lanes and (lanes is not None or B * H * W < 12 * 640 * 640)):
            for o in self.ops:
                o["lane"] = 0

    # ---- split-K (latency mode) ------------------------------------------------------------------------------------
    @staticmethod
    def split_factors(k: int, stride: int, cin: int, c0: int, cout: int, OH: int, OW: int) -> Tuple[int, int]:
        """(channel slices, tap slices) of a dense conv's K walk in latency mode -- a function of the LAYER'S SHAPE ONLY, never of
        the batch: a rank's share of a strong-scaled batch (8 images of 64) and the whole batch cut their K walks at the same places
        and add the partial sums in the same order, so shards of a batch return the bits of the whole.
        Rule (measured, 8 images of 640 x 640, r04: a split costs a second launch and an f32 round trip of the output, ~6 us, so it
        only pays on layers that are long AND thin): at least 32 K-steps of 64, fewer than 11 tiles of 128 x 128 per image, at least
        three slices; 3 x 3 layers are cut by kernel row first, then by 64-channel groups; at most 8 slices, each at least four
        64-deep K-steps.  On YOLO11s that is Detect's cv2.2.0 (3 x 3, 512 -> 64 at 20 x 20: 26.7 -> 16.6 us) and model.20 (19.8 ->
        15.3 us); splitting the 6-10-us 1 x 1 layers of the 20 x 20 stage made each of them 4-8 us SLOWER."""
        if cin % 64 or c0 % 64 or cout % 8:
            return 1, 1
        steps = k * k * cin // 64
        tiles = -(-OH * OW // 128) * -(-cout // 128)
        want = min(32 // max(tiles, 1), 8, steps // 4)
        if steps < 32 or want < 3:
            return 1, 1
        nt = 3 if k == 3 else 1
        n64 = cin // 64
        nc = max((d for d in range(1, n64 + 1) if n64 % d == 0 and d * nt <= want), default=1)
        return (nc, nt) if nc * nt >= 3 else (1, 1)

    def _apply_split_k(self) -> None:
        for o in self.ops:
            if o["kind"] != L.OP_CONV or o.get("out_f32", 0) or o.get("dst_scale", 1) != 1 or o["ksize"] not in (1, 3):
                continue
            s0, s1 = o["src0"], o.get("src1")
            cin = s0.C + (s1.C if s1 else 0)
            cout = o.get("cout", o["dst"].C)
            if o["dst"].ld % 8 or (o.get("res") is not None and o["res"].ld % 8):
                continue
            nc, nt = self.split_factors(o["ksize"], o["stride"], cin, s0.C if s1 else cin, cout, o["OH"], o["OW"])
            if nc * nt < 2:
                continue
            ldw = (cout + 31) // 32 * 32
            self.buf_bytes.append(nc * nt * self.B * o["OH"] * o["OW"] * ldw * 4)
            o["box"] = [T(len(self.buf_bytes) - 1, ldw, 0, ldw, o["OH"], o["OW"], False, True)]
            o["ksplit"] = nc | (nt << 8)

    # ---- buffers -------------------------------------------------------------------------------------------
    def alloc(self, C: int, H: int, W: int, f32: bool = False) -> T:
        if self.f32_mode:
            self.buf_bytes.append(self.B * H * W * make_divisible(C, 8) * 4)
            return T(len(self.buf_bytes) - 1, make_divisible(C, 8), 0, C, H, W, False, True)
        ld = make_divisible(C, 4) if f32 else make_divisible(C, 8)
        self.buf_bytes.append(self.B * H * W * ld * (4 if f32 else 2))
        return T(len(self.buf_bytes) - 1, ld, 0, C, H, W, False, f32)

    def alloc_like(self, x: Union[T, List[T]], C: int) -> T:  # a fresh C-wide map of the size of x, or of a Concat's first operand
        x0 = x[0] if isinstance(x, list) else x
        return self.alloc(C, x0.H, x0.W)

    def stored(self, w: int) -> int:  # the width a piece of w channels is carried on: the fp16 path reads 8-channel pieces
        return w if self.f32_mode else w + -w % 8

    def pieces(self, widths: List[int], H: int, W: int) -> Tuple[T, int]:
        """One map of consecutive pieces of `widths` channels, each carried on its stored() width, zero-padded at its end (T.padded: zero weights
        and bias where it is written, zero weight columns where it is read; no piece needs it: a plain map) -> (map, the first piece's stored width)."""
        w8 = widths if self.f32_mode else [w + -w % 8 for w in widths]  # (stored(), in place: every block of every plan comes through here)
        t = self.alloc(sum(w8), H, W)
        return (t if w8 == widths else t.padded(list(zip(w8, widths)))), w8[0]

    def _fp16_mult8(self, width: int, refusal: str):  # a width the fp16 path cannot carry, where no padded form exists
        if width % 8 and not self.f32_mode:
            raise NotImplementedError(refusal)

    # ---- op emitters -----------------------------------------------------------------------------------------
    def _wrec(self, key: str, **kw) -> str:
        if key not in self.wrecs:
            embed = kw.pop("embed", 0)
            self.wrecs[key] = WRec(**kw)
            if embed:
                self.wrecs[key].embed = embed
        return key

    def _emit(self, kind: int, name: str, flops: int = 0, /, **o) -> dict:
        """The one place an op enters the list: `o` are its fields (OP_FIELDS), `flops` its share of the plan's 2 x MAC count.  H, W
        default to the source's logical size (the destination's where an op has no source), OH, OW to the destination's (H, W where
        it has none); the op runs on the lane that is current.  mfma_flops -- what of `flops` runs on the matrix pipe -- stays in the
        op only where there is any: the benchmark tells the conv family by it.  (Positional-only parameters: a call with fifteen
        keywords is then no dearer than the dict literal it replaces, which keeps plan construction -- on the first forward of every
        new input shape -- where it was.)"""
        assert o.keys() <= OP_FIELDS, f"{name}: unknown op field(s) {sorted(set(o) - OP_FIELDS)}"
        assert not self._lane or kind in LANE_KINDS, f"{name}: an op of kind {kind} on a side lane"
        if "H" not in o:
            t = o["src0"] if o.get("src0") is not None else o["dst"]
            o["H"], o["W"] = t.H, t.W
        if "OH" not in o:
            t = o.get("dst")
            o["OH"], o["OW"] = (t.H, t.W) if t is not None else (o["H"], o["W"])
        if "mfma_flops" in o and not o["mfma_flops"]:
            del o["mfma_flops"]
        o["kind"], o["name"], o["lane"] = kind, name, self._lane
        self.flops += flops
        self.ops.append(o)
        return o

    def conv(self, name: str, src: Union[T, Sequence[T]], cout: int, k: int = 1, s: int = 1, act: Union[bool, int] = True,
             dst: Optional[T] = None, res: Optional[T] = None, plain: bool = False, out_f32: bool = False,
             perm: Optional[List[int]] = None, name2: Optional[str] = None, wkind: Optional[str] = None,
             wshape: Optional[Tuple[int, int, int]] = None, real: Tuple[int, int] = (0, 0),
             rows: Optional[List[int]] = None, cols: Optional[List[int]] = None) -> T:
        """name2: a second Conv module of the same input and kernel whose output channels follow this one's (weights.py
        kind "conv2": the two folded weight matrices stacked along cout) -- one launch for both, cout = the total.
        act: True = the graph's default activation (self.act_id: SiLU, or ReLU under `activation: nn.ReLU()`), False = none, or an
        activation id of include/bsyolo.h itself (SPPF's convs under ReLU name theirs)."""
        srcs = [src] if isinstance(src, T) else list(src)
        assert 1 <= len(srcs) <= 2, "at most two concat operands per conv"
        H, W = srcs[0].H, srcs[0].W
        assert all(t.H == H and t.W == W and (t.f32 == self.f32_mode) for t in srcs)
        if k != 1 and any(t.up for t in srcs):
            # the conv kernels gather nearest x2 for 1x1 convs alone (csrc/conv_select.hip): a 3x3 conv over a Concat whose operand is a
            # virtual Upsample (yolov3-tiny's layer 19, cv1 of YOLOv3's head Bottlenecks) reads that operand from a map of its own,
            # written once by OP_COPY through up0, in every precision
            srcs = [self._materialise(f"{name}.up{j}", t) if t.up else t for j, t in enumerate(srcs)]
        cin = sum(t.C for t in srcs)
        if not self.f32_mode and any(t.C % 8 or t.coff % 8 for t in srcs):
            # csrc/conv_gemm.hip reads its sources in 16-byte (8-channel) pieces; a block whose hidden width is 12 or 20 channels
            # (a C2f / C3k2 of 24 or 40) is refused here rather than at the first launch
            raise NotImplementedError(f"{name}: source channels / offsets {[(t.C, t.coff) for t in srcs]} are not multiples of 8 (fp16 path)")
        p = k // 2
        OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        if dst is None:
            dst = self.alloc(cout, OH, OW, out_f32)
        assert dst.C == cout and dst.H == OH and dst.W == OW and dst.f32 == (out_f32 or self.f32_mode) and not dst.up
        if res is not None:
            assert res.C == cout and res.H == OH and res.W == OW and not res.up
        if rows is None and cols is None and (any(t.cmap is not None for t in srcs) or dst.cmap is not None):
            # padded pieces on either side: the op's weight matrix is the module's with zero rows / columns at the padding channels
            assert perm is None and wshape is None and not real[1]
            out_real = real[0] or dst.real
            rows = list(dst.cmap) if dst.cmap is not None else [i if i < out_real else -1 for i in range(cout)]
            cols, base = [], 0
            for t in srcs:
                cols += [base + v if v >= 0 else -1 for v in (t.cmap if t.cmap is not None else range(t.C))]
                base += t.real
            real = (out_real, base)
            if real[0] < cout and dst.cmap is None:
                dst = dst.padded([(cout, real[0])])
        if name2 is not None:
            assert not plain and perm is None and cout % 2 == 0
            key = self._wrec(name + "+" + name2, name=name, kind="conv2", cout=cout, cin=cin, k=k, post=name2, rows=rows, cols=cols,
                             real_cout=real[0], real_cin=real[1])
        else:
            wc, wi, wk = wshape or (cout, cin, k)  # wshape: the module's own weight shape where the op runs a re-laid-out copy
            key = self._wrec(name, name=name, kind=wkind or ("plain" if plain else "conv"), cout=wc, cin=wi, k=wk, perm=perm,
                             real_cout=real[0], real_cin=real[1], rows=rows, cols=cols)
        fl = 2 * self.B * OH * OW * cout * cin * k * k
        self._emit(L.OP_CONV, name, fl, src0=srcs[0], src1=srcs[1] if len(srcs) > 1 else None, dst=dst, res=res, ksize=k, stride=s, pad=p,
                   act=self.act_id if act is True else int(act), out_f32=int(out_f32), wkey=key, dst_scale=1, cout=cout, mfma_flops=fl)
        return dst

    def conv_first(self, name: str, cout: int, k: int, s: int, p: Optional[int] = None) -> T:
        p = k // 2 if p is None else p
        img = self._ext("im", self.EXT_IMG, 3, (self.H, self.W))
        if (k, s, p) == (6, 2, 2) and not self.f32_mode:
            # YOLOv5u's stem (cfg/models/v5/yolov5.yaml:16): space-to-depth of the image (one elementwise launch) + an ordinary
            # 3x3 stride-1 conv over its 12 (+4 zero) channels with the weights re-laid-out to match (weights.py "first_s2d")
            assert self.H % 2 == 0 and self.W % 2 == 0
            sd = self.alloc(16, self.H // 2, self.W // 2)
            self._emit(L.OP_S2D, name + ".s2d", src0=img, dst=sd, in_dtype=self.in_dtype)
            return self.conv(name, sd, cout, 3, 1, wkind="first_s2d", wshape=(cout, 3, 6))
        OH, OW = (self.H + 2 * p - k) // s + 1, (self.W + 2 * p - k) // s + 1
        dst = self.alloc(cout, OH, OW)
        key = self._wrec(name, name=name, kind="first", cout=cout, cin=3, k=k)
        fl = 2 * self.B * OH * OW * cout * 3 * k * k
        self._emit(L.OP_CONV_FIRST, name, fl, src0=img, dst=dst, ksize=k, stride=s, pad=p, act=self.act_id, wkey=key, in_dtype=self.in_dtype,
                   mfma_flops=fl)
        return dst

    def dwconv(self, name: str, src: T, act: bool, dst: Optional[T] = None, res: Optional[T] = None, real_c: int = 0) -> T:
        assert not src.up
        if dst is None:
            dst = self.alloc(src.C, src.H, src.W)
        key = self._wrec(name, name=name, kind="dw", cout=src.C, cin=1, k=3, real_cout=real_c)
        self._emit(L.OP_DWCONV, name, 2 * self.B * src.H * src.W * src.C * 9,
                   src0=src, dst=dst, res=res, ksize=3, stride=1, pad=1, act=int(act), wkey=key)
        return dst

    def dwconv_g(self, name: str, src: T, kh: int, kw: int, s: int, act_c: int, dst: Optional[T] = None, kind: str = "dwg",
                 post: Optional[str] = None, rows: Optional[List[int]] = None, real_c: int = 0) -> T:
        """Depthwise kh x kw conv with "same" padding (csrc/bsyolo_ops.hip); SiLU on the first act_c channels.
        kind: "dwg" (Conv + BN), "dwg_plain" (bare nn.Conv2d with bias), "dwg_ext" (PMSFA.conv3, see pmsfa())."""
        assert not src.up and src.f32 == self.f32_mode
        OH, OW = (src.H + 2 * (kh // 2) - kh) // s + 1, (src.W + 2 * (kw // 2) - kw) // s + 1
        if dst is None:
            dst = self.alloc(src.C, OH, OW)
        assert dst.C == src.C and dst.H == OH and dst.W == OW
        key = self._wrec(name, name=name, kind=kind, cout=src.C, cin=1, k=kh, kw=kw, post=post, rows=rows, real_cout=real_c)
        self._emit(L.OP_DWCONV_G, name, 2 * self.B * OH * OW * src.C * kh * kw,
                   src0=src, dst=dst, ksize=kh, pad=kw, stride=s, act=int(act_c), wkey=key, heads=src.C, key_dim=0,
                   mid_c=src.C // 2 if kind == "dwg_ext" else 0)  # first channel of the identity-kernel half
        return dst

    def dwpw(self, name: str, src: T, cout: int, real: Tuple[int, int] = (0, 0), parts: Tuple[str, str] = ("0", "1")) -> T:
        """nn.Sequential(DWConv(c, c, 3), Conv(c, cout, 1)) (head.py:49-57): one fused launch where dwpw_fused.hip's
        dwpw_fused_kernel takes the widths, else the two ordinary launches.  real = the modules' own (cout, cin) where `cout` / `src`
        are padded to a multiple of 8.  parts: the two modules' names under `name` (CIB's second pair is "2", "3")."""
        nd, npw = f"{name}.{parts[0]}", f"{name}.{parts[1]}"
        if not (self.fuse_dwpw and kernel_takes("dwpw_fused", src.C, cout) and not src.up and src.cmap is None):
            t = self.dwconv(nd, src, act=True, real_c=real[1])
            return self.conv(npw, t, cout, 1, 1, real=real)
        kd = self._wrec(nd, name=nd, kind="dw", cout=src.C, cin=1, k=3, real_cout=real[1])
        kp = self._wrec(npw, name=npw, kind="conv", cout=cout, cin=src.C, k=1, perm=None, real_cout=real[0], real_cin=real[1])
        dst = self.alloc(cout, src.H, src.W)
        px = 2 * self.B * src.H * src.W * src.C
        self._emit(L.OP_DWPW, name, px * (9 + cout), src0=src, dst=dst, ksize=3, stride=1, pad=1, act=1, wkey=kd, wkey2=kp,
                   mfma_flops=px * cout)  # the dense 1x1 part (the depthwise is VALU work)
        return dst

    def copy(self, name: str, src: T, dst: T):
        assert dst.C == src.C and dst.H == src.H and dst.W == src.W and not dst.up
        self._emit(L.OP_COPY, name, src0=src, dst=dst)

    def _materialise(self, name: str, src: T) -> T:
        """The full-size map of a virtual nearest x2 Upsample view, written by one OP_COPY the first time a consumer needs it."""
        key = (src.buf, src.coff, src.C)
        if key not in self._up_real:
            real = self.alloc(src.C, src.H, src.W)
            real.cmap = src.cmap
            self.copy(name, src, real)
            self._up_real[key] = real
        return self._up_real[key]

    def maxpool(self, name: str, src: T, mode: int) -> T:
        """csrc/maxpool.hip.  mode 0: nn.MaxPool2d(2, 2, 0) on an even map; mode 1: nn.ZeroPad2d((0, 1, 0, 1)) + nn.MaxPool2d(2, 1, 0), the
        padded taps counting as 0.0."""
        if src.up or src.cmap is not None:
            raise NotImplementedError(f"{name}: a max pool over an upsampled or zero-padded view is not accelerated")
        if mode == 0 and (src.H % 2 or src.W % 2 or src.H < 2 or src.W < 2):
            raise NotImplementedError(f"{name}: MaxPool2d(2, 2, 0) on an odd {src.H} x {src.W} map is not accelerated")
        v = 4 if self.f32_mode else 8
        if src.C % v or src.coff % v:
            raise NotImplementedError(f"{name}: {src.C} channels at offset {src.coff} are not multiples of {v}")
        dst = self.alloc(src.C, *((src.H, src.W) if mode else (src.H // 2, src.W // 2)))
        self._emit(L.OP_MAXPOOL, name, src0=src, dst=dst, level=mode, ksize=2, stride=1 if mode else 2, pad=0)
        return dst

    def top_bottleneck(self, name: str, x: Union[T, List[T]], c2: int, shortcut: bool, k=(3, 3), e: float = 0.5) -> T:
        """A Bottleneck as a top-level layer (YOLOv3's darknet-53 and its head; block.py:3405-3419).  A two-operand Concat goes to cv1 as two
        sources; the identity shortcut exists where c1 == c2 (:3413), which a Concat input of the shipped graphs never has."""
        if isinstance(x, T):
            dst = self.alloc_like(x, c2)
            self.bottleneck(name, x, dst, shortcut, k, e)
            return dst
        c_ = int(c2 * e)
        if shortcut and sum(t.C for t in x) == c2:
            raise NotImplementedError(f"{name}: a Bottleneck with a shortcut over a Concat is not accelerated")
        self._fp16_mult8(c_, f"{name}: a Bottleneck with a hidden width of {c_} channels over a Concat is not on the fp16 path (multiples of 8)")
        t = self.conv(name + ".cv1", x, c_, k[0], 1)
        return self.conv(name + ".cv2", t, c2, k[1], 1)

    # ---- module expansions -----------------------------------------------------------------------------------
    def bottleneck(self, name: str, x: T, dst: T, shortcut: bool, k=(3, 3), e=0.5, rep: bool = False):
        """block.py:3405-3419: x + cv2(cv1(x)).  rep: a RepBottleneck (:3634-3641) -- cv1 is a RepConv, in the form self.repconv names: one
        3x3 conv either way once the host has folded it (weights.py kinds "refconv": no activation, zero bias; "repvgg": SiLU).  The
        one-launch Bottleneck kernel computes SiLU after cv1 and is built for e = 0.5, so it serves neither (a RepBottleneck has e = 1)."""
        c_ = int(dst.real * e)
        cv1 = dict(act=self.repconv == "repvgg", wkind=self.repconv) if rep else {}
        if (not rep and self.fuse_bneck and tuple(k) == (3, 3) and shortcut and x.C == dst.C and not x.up and not x.f32 and x.cmap is None and dst.cmap is None
                and kernel_takes("bottleneck_fused", x.C, c_)):
            # one launch, hidden map kept in LDS (csrc/bneck_fused.hip)
            k1 = self._wrec(name + ".cv1", name=name + ".cv1", kind="conv", cout=c_, cin=x.C, k=3, perm=None)
            k2 = self._wrec(name + ".cv2", name=name + ".cv2", kind="conv", cout=dst.C, cin=c_, k=3, perm=None)
            fl = 2 * self.B * x.H * x.W * 9 * 2 * c_ * x.C
            self._emit(L.OP_BNECK, name, fl, src0=x, dst=dst, ksize=3, stride=1, pad=1, act=1, wkey=k1, wkey2=k2, mid_c=c_, mfma_flops=fl)
            return
        res = x if (shortcut and x.C == dst.C) else None
        if c_ % 8 and not self.f32_mode:
            # hidden width 4 / 12 / 20 (a C3k2 of 16 / 48 / 80 channels with e = 0.25 x 0.5, e.g. YOLO11 at width 0.125 / 0.375): the
            # hidden map is carried on the next multiple of 8 with zero weights and bias in the padding (weights.py real_cout /
            # real_cin, as Detect's class branch does for nc-dependent widths) -- SiLU(0) = 0 there, the real channels are unchanged
            if x.cmap is not None or dst.cmap is not None:  # inside a block whose chunks are padded pieces themselves (c2f below)
                t, c8 = self.pieces([c_], x.H, x.W)
                t = self.conv(name + ".cv1", x, c8, k[0], 1, dst=t, **cv1)
                self.conv(name + ".cv2", t, dst.C, k[1], 1, dst=dst, res=res)
                return
            c8 = self.stored(c_)
            t = self.conv(name + ".cv1", x, c8, k[0], 1, real=(c_, 0), **cv1)
            self.conv(name + ".cv2", t, dst.C, k[1], 1, dst=dst, res=res, real=(0, c_))
            return
        t = self.conv(name + ".cv1", x, c_, k[0], 1, **cv1)
        self.conv(name + ".cv2", t, dst.C, k[1], 1, dst=dst, res=res)

    def cib(self, name: str, x: T, dst: T, shortcut: bool, lk: bool):
        """block.py:4176-4212 CIB(c, c, shortcut, e = 1.0, lk), the block of C2fCIB: x + cv1(x), cv1 a Sequential of five Convs, SiLU after each --
        0: depthwise 3x3 (c); 1: 1x1 (c -> 2c); 2: depthwise 3x3 (2c), or with lk RepVGGDW (2c): a depthwise 7x7 once folded (weights.py
        kind "repvggdw"); 3: 1x1 (2c -> c); 4: depthwise 3x3 (c).  Lowered as dwpw(0 + 1), dwpw(2 + 3) -- with lk DWCONV_G 7x7, then CONV --
        and DWCONV(4) with x as its shortcut, written into the C2f piece.  A piece carried on the next multiple of 8 (T.cmap: c = 12,
        20 ...; 2c is a multiple of 8 whenever c2 is) takes the two-launch forms, with zero weights and biases in its padding."""
        c = dst.real
        assert x.real == c and x.C == dst.C and not x.up
        n, padded = name + ".cv1", x.cmap is not None or dst.cmap is not None
        if padded:
            t = self.dwconv(n + ".0", x, act=True, dst=self.pieces([c], x.H, x.W)[0], real_c=c)
            t = self.conv(n + ".1", t, 2 * c, 1, 1)
        else:
            t = self.dwpw(n, x, 2 * c)
        if lk or padded:
            t = self.dwconv_g(n + ".2", t, 7, 7, 1, 2 * c, kind="repvggdw") if lk else self.dwconv(n + ".2", t, act=True)
            t = self.conv(n + ".3", t, dst.C, 1, 1, dst=self.pieces([c], x.H, x.W)[0] if padded else None)
        else:
            t = self.dwpw(n, t, dst.C, parts=("2", "3"))
        self.dwconv(n + ".4", t, act=True, dst=dst, res=x if shortcut else None, real_c=c if t.cmap is not None else 0)

    def ghostconv(self, name: str, src: Union[T, Sequence[T]], c2: int, k: int = 1, s: int = 1, act: bool = True, dst: Optional[T] = None,
                  res: Optional[T] = None) -> T:
        """conv.py:280-293 GhostConv: cat(y, cv2(y)) with y = cv1(x), cv1 = Conv(c1, c2 // 2, k, s, act), cv2 = Conv(c2 // 2, c2 // 2, 5, 1,
        g = c2 // 2, act), depthwise.  res: a shortcut operand added to the concat (GhostBottleneck).  One OP_GHOST where cv1 is 1x1
        stride 1 on one plain source and the kernel takes the widths; else cv1 and cv2 as CONV and DWCONV_G into the halves of one
        buffer, which with a shortcut is a scratch buffer that OP_ADD adds `res` to.  fp16 path, c2 // 2 not a multiple of 8: both halves
        are carried on the next multiple of 8 as zero-padded pieces (T.cmap), as c2f / c3k carry their chunks."""
        srcs = [src] if isinstance(src, T) else list(src)
        if c2 % 2:
            raise NotImplementedError(f"{name}: GhostConv with {c2} output channels does not split into two halves")
        if k not in (1, 3) or s not in (1, 2):
            raise NotImplementedError(f"{name}: GhostConv with k={k} s={s} (cv1 is accelerated for k 1 / 3, stride 1 / 2)")
        hr = c2 // 2  # the module's hidden width
        CH = self.stored(hr)
        pad = CH != hr
        p = k // 2
        OH, OW = (srcs[0].H + 2 * p - k) // s + 1, (srcs[0].W + 2 * p - k) // s + 1
        if dst is None:
            dst = self.pieces([hr, hr], OH, OW)[0]
        assert dst.C == 2 * CH and dst.H == OH and dst.W == OW and (res is None or res.C == dst.C)
        fuse = (self.fuse_ghost and k == 1 and s == 1 and len(srcs) == 1 and not srcs[0].up and not srcs[0].C % 8 and not srcs[0].coff % 8
                and kernel_takes("ghost_fused", srcs[0].C, CH))
        pair = dst if res is None or fuse else self.pieces([hr, hr], OH, OW)[0]
        first = len(self.ops)
        y = self.conv(name + ".cv1", srcs[0] if len(srcs) == 1 else srcs, CH, k, s, act=act, dst=pair.slice(0, CH))
        self.dwconv_g(name + ".cv2", y, 5, 5, 1, CH if act else 0, dst=pair.slice(CH, CH),
                      rows=[i if i < hr else -1 for i in range(CH)] if pad else None, real_c=hr if pad else 0)
        if fuse:
            # the two launches just listed become one: their weight records (the unfused plan's, in its order) and their flops stay
            cv1, cv2 = self.ops[first:]
            del self.ops[first:]
            self._emit(L.OP_GHOST, name, src0=srcs[0], dst=dst, res=res, ksize=5, stride=1, pad=2, act=int(act), mid_c=CH, wkey=cv1["wkey"],
                       wkey2=cv2["wkey"], mfma_flops=cv1["mfma_flops"])  # the dense 1x1 part (the depthwise is VALU work)
        elif res is not None:
            self._emit(L.OP_ADD, name + ".add", src0=pair, src1=res, dst=dst)
        return dst

    def ghost_bottleneck(self, name: str, x: T, dst: T, s: int = 1):
        """block.py:3384-3402 with s = 1 (the only form the reference's yamls reach): x + GhostConv(c2 // 2, c2, 1, 1, act=False)(GhostConv(c1,
        c2 // 2, 1, 1)(x)); nn.Sequential names the two `conv.0` and `conv.2`.  The first GhostConv's hidden width is c2 // 4 (zero-padded
        pieces where that is 4, 12, 20 ...), the second's c2 // 2."""
        if s != 1:
            raise NotImplementedError(f"{name}: GhostBottleneck with s = {s} (its depthwise stride-2 form is in no shipped graph) is not accelerated")
        c2 = dst.real
        if x.real != c2 or c2 % 4:
            raise NotImplementedError(f"{name}: GhostBottleneck {x.real} -> {c2} (the identity shortcut needs equal widths, the halves a multiple of 4)")
        c_ = c2 // 2
        self._fp16_mult8(c_, f"{name}: GhostBottleneck with a hidden width of {c_} channels is not on the fp16 path (multiples of 8)")
        t = self.ghostconv(name + ".conv.0", x, c_, 1, 1, True)
        self.ghostconv(name + ".conv.2", t, c2, 1, 1, False, dst=dst, res=x)

    def c3k(self, name: str, x, dst: T, n: int, shortcut: bool, k=(3, 3), rep: bool = False, ghost: bool = False):
        """block.py:3320-3334 + :3807-3815: cv3(cat(m(cv1 x), cv2 x)), m = n x Bottleneck(c_, c_, k=(3,3), e=1); C3 itself
        (YOLOv5u) is the same with k = ((1,1), (3,3)) and may read a two-operand Concat.  rep: RepCSP (:3644-3651), the same block
        over RepBottlenecks.  ghost: C3Ghost (:3374-3381), the same block over GhostBottleneck(c_, c_)."""
        cr = int(dst.real * 0.5)  # the module's hidden width
        x0 = x if isinstance(x, T) else x[0]
        # fp16 path, hidden width not a multiple of 8 (a C3k of 12 / 20 / 24 channels ...): both halves of the concat are zero-padded pieces
        cat, c_ = self.pieces([cr, cr], x0.H, x0.W)
        if self.merge_c3k and n >= 2:
            # cv1 and cv2 read the same x: ONE launch writes [cv1 x | cv2 x] into the concat buffer (twice the cout per
            # pixel tile, one launch less); the last bottleneck then overwrites the cv1 half, which only the first one reads
            self.conv(name + ".cv1", x, 2 * c_, 1, 1, dst=cat, name2=name + ".cv2")
            cur = cat.slice(0, c_)
        else:
            cur = self.conv(name + ".cv1", x, c_, 1, 1, dst=self.pieces([cr], x0.H, x0.W)[0])
            self.conv(name + ".cv2", x, c_, 1, 1, dst=cat.slice(c_, c_))
        for i in range(n):
            out = cat.slice(0, c_) if i == n - 1 else self.pieces([cr], x0.H, x0.W)[0]
            if ghost:
                self.ghost_bottleneck(f"{name}.m.{i}", cur, out)
            else:
                self.bottleneck(f"{name}.m.{i}", cur, out, shortcut, k, 1.0, rep=rep)
            cur = out
        self.conv(name + ".cv3", cat, dst.C, 1, 1, dst=dst)

    def c2f(self, name: str, x, c2: int, n: int, shortcut: bool, e: float, inner: str, lk: bool = False) -> T:
        """block.py:3295-3317 (C2f) / :3796-3804 (C3k2) / :4215-4232 (C2fCIB).  inner: 'c2f' | 'bottleneck' | 'c3k' | 'cib' (with `lk`: CIB's RepVGGDW)."""
        xs = [x] if isinstance(x, T) else list(x)
        c = int(c2 * e)
        if (self.fuse_tail and inner == "bottleneck" and n == 1 and shortcut and len(xs) == 1 and not xs[0].up and not xs[0].f32
                and kernel_takes("c3k2_fused", xs[0].C, c, c2)):
            # the whole block in one launch (csrc/c3k2_fused.hip): x in, out out, the [y0 | y1 | y2] concat never reaches HBM
            names = [name + ".cv1", name + ".m.0.cv1", name + ".m.0.cv2", name + ".cv2"]
            shapes = [(2 * c, xs[0].C, 1), (c // 2, c, 3), (c, c // 2, 3), (c2, 3 * c, 1)]
            keys = [self._wrec(nm, name=nm, kind="conv", cout=co, cin=ci, k=k, perm=None) for nm, (co, ci, k) in zip(names, shapes)]
            dst = self.alloc_like(xs, c2)
            fl = 2 * self.B * xs[0].H * xs[0].W * sum(co * ci * k * k for co, ci, k in shapes)
            self._emit(L.OP_C3K2, name, fl, src0=xs[0], dst=dst, ksize=3, stride=1, pad=1, act=1, wkeys=keys, mid_c=c, mfma_flops=fl)
            return dst
        # fp16 path, chunk width not a multiple of 8 (c = 12 / 20 ...; tasks.py:1016 scales c2 by any width multiple): every chunk of the
        # concat is carried on the next multiple of 8 as a zero-padded piece (T.cmap) -- cv1 writes zero rows there, cv2 reads zero columns
        padded = inner in ("bottleneck", "c2f", "c3k", "cib")  # (PMSFA refuses such a width itself)
        cat, c = self.pieces([c] * (2 + n), xs[0].H, xs[0].W) if padded else (self.alloc_like(xs, (2 + n) * c), c)
        self.conv(name + ".cv1", xs, 2 * c, 1, 1, dst=cat.slice(0, 2 * c))
        for i in range(n):
            src, dst = cat.slice((1 + i) * c, c), cat.slice((2 + i) * c, c)
            if inner == "pmsfa":
                self.pmsfa(f"{name}.m.{i}", src, dst)
            elif inner == "c3k_gai":
                self.c3k_gai(f"{name}.m.{i}", src, dst, 2)
            elif inner == "c3k":
                self.c3k(f"{name}.m.{i}", src, dst, 2, shortcut)
            elif inner == "cib":
                self.cib(f"{name}.m.{i}", src, dst, shortcut, lk)
            elif inner == "c2f":
                self.bottleneck(f"{name}.m.{i}", src, dst, shortcut, (3, 3), 1.0)
            else:
                self.bottleneck(f"{name}.m.{i}", src, dst, shortcut, (3, 3), 0.5)
        return self.conv(name + ".cv2", cat, c2, 1, 1)

    def c2(self, name: str, x, c2: int, n: int, shortcut: bool) -> T:
        """block.py:3277-3292 (C2): cv2(cat(m(a), b)) with [a | b] = cv1(x), m = n x Bottleneck(c, c, k=(3,3), e=1).  cv2 reads
        the two halves as a virtual concat (a two-source conv): m's output in a buffer of its own, b where cv1 left it."""
        xs = [x] if isinstance(x, T) else list(x)
        c = int(c2 * 0.5)
        self._fp16_mult8(c, f"{name}: C2 with a hidden width of {c} channels is not on the fp16 path (multiples of 8)")
        ab = self.alloc_like(xs, 2 * c)
        self.conv(name + ".cv1", xs, 2 * c, 1, 1, dst=ab)
        cur = ab.slice(0, c)
        for i in range(n):
            out = self.alloc_like(xs, c)
            self.bottleneck(f"{name}.m.{i}", cur, out, shortcut, (3, 3), 1.0)
            cur = out
        return self.conv(name + ".cv2", [cur, ab.slice(c, c)], c2, 1, 1)

    def c2f_attn(self, name: str, x, c2: int, n: int, ec: int, nh: int) -> T:
        """block.py:3518-3535 C2fAttn(c1, c2, n, ec, nh): cv2(cat(y0, y1, m(y1) ..., attn(y[-1], guide))), [y0 | y1] = cv1(x), m = n x
        Bottleneck(c, c, shortcut False, k=(3,3), e=1), attn = MaxSigmoidAttnBlock(c, c, gc=512, ec, nh) (:3483-3515): proj_conv (3x3, BN, no
        activation) of the last chunk, every head's channels multiplied by scale * sigmoid(max over the classes of <embedding, guide row> /
        sqrt(hc) + bias).  One concat buffer of 3 + n chunks as c2f's; proj_conv writes the last chunk and ONE MAXSIG op gates it in place,
        its embedding the chunk before.  The guide -- gl (nn.Linear(512, ec)) applied to the text features, constant per call -- is folded
        on the host (weights.py kind "maxsig").  An `attn.ec` conv would exist where ec != c, and the module's own views then do not fit
        (embed.view(bs, nh, hc, h, w) needs ec = nh * hc = c): no stock scale has one, and it is refused."""
        xs = [x] if isinstance(x, T) else list(x)
        c = int(c2 * 0.5)
        if nh < 1 or c % nh:
            raise NotImplementedError(f"{name}: C2fAttn with {nh} heads on {c} channels (the heads must divide the hidden width)")
        hc = c // nh
        if ec != c:
            raise NotImplementedError(f"{name}: C2fAttn with ec = {ec} != c = {c} (attn.ec, a 1x1 conv to a width the module's own views do not fit) is not accelerated")
        if not self.f32_mode and not kernel_takes("maxsig", hc):
            raise NotImplementedError(f"{name}: C2fAttn heads of hc = {hc} channels are not on the fp16 path (16 to 128 in steps of 16)")
        H, W = xs[0].H, xs[0].W
        cat, cs = self.pieces([c] * (3 + n), H, W)
        assert cs == c and cat.cmap is None  # (fp16: c = nh * hc is a multiple of 16)
        self.conv(name + ".cv1", xs, 2 * c, 1, 1, dst=cat.slice(0, 2 * c))
        for i in range(n):
            self.bottleneck(f"{name}.m.{i}", cat.slice((1 + i) * c, c), cat.slice((2 + i) * c, c), False, (3, 3), 1.0)
        emb, gated = cat.slice((1 + n) * c, c), cat.slice((2 + n) * c, c)
        self.conv(name + ".attn.proj_conv", emb, c, 3, 1, act=False, dst=gated)
        tnc = self.text_nc or self.cfg["nc"]
        key = self._wrec(name + ".attn", name=name + ".attn", kind="maxsig", cout=tnc, cin=c, k=nh, embed=512)  # (gc = 512: C2fAttn's default)
        self._emit(L.OP_MAXSIG, name + ".attn", 2 * self.B * H * W * c * tnc, src0=emb, src1=gated, dst=gated, heads=nh, head_dim=hc, nc=tnc, wkey=key)
        return self.conv(name + ".cv2", cat, c2, 1, 1)

    def pmsfa(self, name: str, x: T, dst: T):
        """block.py:3035-3054.  conv1 -> P = [p1 | p2]; depthwise 5x5 on p1 -> Q = [q1 | q2]; the depthwise 7x7 runs on ALL
        of Q with weights extended by an identity kernel for the q2 half (weights.py kind "dwg_ext": exact pass-through,
        SiLU only on the q1 half) -> S = [conv3(q1) | q2]; conv4 reads the virtual concat [S | p2] = the reference's
        cat([conv3_out, conv2_out_2, conv1_out_2]) and adds x."""
        c = x.C
        assert dst.C == c
        if c % 4:  # the reference's constructor needs it too (Conv(inc // 4, inc // 4, 7, g=inc // 4) on half of a half)
            raise NotImplementedError(f"PMSFA width {c}: must be a multiple of 4")
        if c % 8 and not self.f32_mode:  # the fp16 conv kernels read their sources in 8-channel pieces (so do the blocks around a PMSFA)
            raise NotImplementedError(f"PMSFA width {c}: must be a multiple of 8 on the fp16 path")
        if c % 16:
            return self._pmsfa_padded(name, x, dst)
        P = self.conv(name + ".conv1", x, c, 3, 1)
        if self.fuse_pmsfa and kernel_takes("pmsfa_tail", c) and not x.up:
            # everything after conv1 in one launch: the map is read once and written once (csrc/pmsfa_fused.hip); the weight records are
            # the unfused plan's, in its order (blob layout, synth_state_dict's random draws)
            k2 = self._wrec(name + ".conv2", name=name + ".conv2", kind="dwg", cout=c // 2, cin=1, k=5, kw=5, post=None, rows=None, real_cout=0)
            k3 = self._wrec(name + ".conv3", name=name + ".conv3", kind="dwg_ext", cout=c // 2, cin=1, k=7, kw=7, post=None, rows=None, real_cout=0)
            k4 = self._wrec(name + ".conv4", name=name + ".conv4", kind="conv", cout=c, cin=c, k=1, perm=None)
            px = 2 * self.B * x.H * x.W
            self._emit(L.OP_PMSFA_TAIL, name + ".tail", px * (c // 2 * 25 + c // 2 * 49 + c * c),  # what the three launches count
                       src0=P, res=x, dst=dst, ksize=1, stride=1, pad=0, act=1, wkeys=[k2, k3, k4], heads=c // 2, key_dim=c // 2,
                       mfma_flops=px * c * c)  # the 1x1
            return
        Q = self.dwconv_g(name + ".conv2", P.slice(0, c // 2), 5, 5, 1, c // 2)
        # S overwrites p1 (dead once conv2 has read it): conv4 then reads ONE contiguous source [S | p2] = P -- at c = 32 two 16-channel
        # sources put it on the unaligned configuration (0.10 ms at 160 x 160, B = 64); same K order, same bits
        S = self.dwconv_g(name + ".conv3", Q, 7, 7, 1, c // 4, kind="dwg_ext", dst=P.slice(0, c // 2))
        self.conv(name + ".conv4", P, c, 1, 1, dst=dst, res=x)

    def _pmsfa_padded(self, name: str, x: T, dst: T):
        """PMSFA on a width that is not a multiple of 16: the depthwise kernels work on 8-channel pieces, so the three pieces of
        conv1's output -- p1a, p1b (the halves of the depthwise 5x5's input) and p2 -- each start at a multiple of 8: conv1 writes
        P' = [p1a 0.. | p1b 0.. | p2 0..] (weights.py `rows`: zero weights and bias in the padding, so the padding channels are
        SiLU(0) = 0 and stay 0 through the depthwise convs), and conv4 reads [S' | p2'] with zero weights on the padding (`cols`).
        The real channels see exactly the reference's arithmetic."""
        c = x.C
        q, h = c // 4, c // 2
        Q8, H8 = make_divisible(q, 8), make_divisible(h, 8)
        pad = lambda real, width, base: [base + i if i < real else -1 for i in range(width)]
        lay = pad(q, Q8, 0) + pad(q, Q8, q) + pad(h, H8, h)           # P' channel -> conv1 output channel
        P = self.conv(name + ".conv1", x, len(lay), 3, 1, rows=lay, real=(c, 0))
        Q = self.dwconv_g(name + ".conv2", P.slice(0, 2 * Q8), 5, 5, 1, 2 * Q8, rows=pad(q, Q8, 0) + pad(q, Q8, q), real_c=h)
        S = self.dwconv_g(name + ".conv3", Q, 7, 7, 1, Q8, kind="dwg_ext", rows=pad(q, Q8, 0), real_c=q, dst=P.slice(0, 2 * Q8))
        self.conv(name + ".conv4", P, c, 1, 1, dst=dst, res=x, cols=lay, real=(0, c))

    def c3k_gai(self, name: str, x: T, dst: T, n: int):
        """block.py:3079-3086: C3 (cv3(cat(m(cv1 x), cv2 x))) with m = n x PMSFA(c_)."""
        c_ = int(dst.C * 0.5)
        cat = self.alloc(2 * c_, x.H, x.W)
        cur = self.conv(name + ".cv1", x, c_, 1, 1)
        self.conv(name + ".cv2", x, c_, 1, 1, dst=cat.slice(c_, c_))
        for i in range(n):
            out = cat.slice(0, c_) if i == n - 1 else self.alloc(c_, x.H, x.W)
            self.pmsfa(f"{name}.m.{i}", cur, out)
            cur = out
        self.conv(name + ".cv3", cat, dst.C, 1, 1, dst=dst)

    def scdown(self, name: str, x: T, c2: int, k: int, s: int) -> T:
        """block.py:4503-4535."""
        t = self.conv(name + ".cv1", x, c2, 1, 1)
        return self.dwconv_g(name + ".cv2", t, k, k, s, 0)

    def msca(self, name: str, x: T) -> T:
        """nn/Addmodules/MSCA.py:19-88.  The depthwise 1x1 `dilconv` that follows the first three branches' column convs is
        folded into their weights; the four SE convs run on (B, 1, 1, C) maps through the ordinary 1x1 conv kernel."""
        assert not x.up
        C, H, W = x.C, x.H, x.W
        strips = ((5, "conv0"), (7, "conv1"), (11, "conv2"), (21, "conv3"))
        branches, logits = [], []
        if self.fuse_msca and kernel_takes("msca_spatial", H, W):
            # one launch for the nine depthwise convs and the four global means (csrc/bsyolo_ops.hip msca_spatial_kernel)
            keys = [self._wrec(name + ".conv0", name=name + ".conv0", kind="dwg_plain", cout=C, cin=1, k=5, kw=5)]
            for i, (k, base) in enumerate(strips):
                keys.append(self._wrec(f"{name}.{base}_1", name=f"{name}.{base}_1", kind="dwg_plain", cout=C, cin=1, k=1, kw=k))
                keys.append(self._wrec(f"{name}.{base}_2", name=f"{name}.{base}_2", kind="dwg_plain", cout=C, cin=1, k=k, kw=1,
                                       post=(name + ".dilconv") if i < 3 else None))
                se = f"{name}.SE{i + 1}.conv.0"  # registered here so the records keep the unfused plan's order (blob layout,
                self._wrec(se, name=se, kind="plain", cout=C, cin=C, k=1, perm=None)  # synth_state_dict's random draws)
            branches = [self.alloc(C, H, W) for _ in strips]
            gaps = [self.alloc(C, 1, 1) for _ in strips]
            self._emit(L.OP_MSCA_SPATIAL, name + ".spatial", 2 * self.B * H * W * C * (25 + 2 * sum(k for k, _ in strips)),
                       src0=x, box=branches[:3], res=branches[3], cls=gaps[:3], msk=[gaps[3]], wkeys=keys)
            for i, g in enumerate(gaps):
                logits.append(self.conv(f"{name}.SE{i + 1}.conv.0", g, C, 1, 1, act=False, plain=True, out_f32=True))
        else:
            attn = self.dwconv_g(name + ".conv0", x, 5, 5, 1, 0, kind="dwg_plain")
            for i, (k, base) in enumerate(strips):
                a = self.dwconv_g(f"{name}.{base}_1", attn, 1, k, 1, 0, kind="dwg_plain")
                a = self.dwconv_g(f"{name}.{base}_2", a, k, 1, 1, 0, kind="dwg_plain", post=(name + ".dilconv") if i < 3 else None)
                branches.append(a)
                g = self.alloc(C, 1, 1)
                self._emit(L.OP_GAP, f"{name}.gap{i}", src0=a, dst=g)
                logits.append(self.conv(f"{name}.SE{i + 1}.conv.0", g, C, 1, 1, act=False, plain=True, out_f32=True))
        mix = self.alloc(C, H, W)
        self._emit(L.OP_MSCA_MIX, name + ".mix", dst=mix, box=branches[:3], res=branches[3], cls=logits[:3], msk=[logits[3]])
        t = self.conv(name + ".conv4", mix, C, 1, 1, act=False, plain=True)
        out = self.alloc(C, H, W)
        self._emit(L.OP_MUL, name + ".mul", src0=t, src1=x, dst=out)
        return out

    def ela(self, name: str, x: T) -> T:
        """nn/Addmodules/ELA.py:33-101."""
        assert not x.up
        if x.C % 8 or x.C % max(1, x.C // 16):  # GroupNorm(max(1, C // 16), C): the reference's constructor needs the second
            raise NotImplementedError(f"ELA on {x.C} channels: must be a multiple of 8 that splits into {x.C // 16} groups")
        k = int(abs((math.log(x.C, 2) + 1) / 2))
        k = k if k % 2 else k + 1
        key = self._wrec(name, name=name, kind="ela", cout=x.C, cin=1, k=k)
        self.buf_bytes.append(self.B * (2 * (x.H + x.W) + 2) * x.C * 4)
        scratch = T(len(self.buf_bytes) - 1, x.C, 0, x.C, 1, 1, False, True)
        dst = self.alloc(x.C, x.H, x.W)
        self._emit(L.OP_ELA, name, src0=x, dst=dst, res=scratch, ksize=k, wkey=key)
        return dst

    def sppf(self, name: str, x: T, c2: int, c_: Optional[int] = None, last: str = "cv2") -> T:
        """block.py:3114-3149.  SPPELAN (:3726-3743) is the same dataflow with the hidden width c_ from the yaml and the last conv
        named cv5."""
        c_ = x.C // 2 if c_ is None else c_
        # under a ReLU graph the two convs follow sppf_act (__init__), not the graph's default
        act = (L.ACT_RELU if self.sppf_act == "relu" else L.ACT_SILU) if self.act_id == L.ACT_RELU else True
        cat = self.alloc(4 * c_, x.H, x.W)
        self.conv(name + ".cv1", x, c_, 1, 1, act=act, dst=cat.slice(0, c_))
        self._emit(L.OP_SPPF_POOL, name + ".m", src0=cat.slice(0, c_))
        return self.conv(name + "." + last, cat, c2, 1, 1, act=act)

    # ---- YOLOv9 (GELAN) blocks --------------------------------------------------------------------------------------
    def pool_down(self, name: str, src: T, mode: int) -> T:
        """The pooling in front of AConv / ADown's convs (csrc/pool_down.hip).  mode 0: avg_pool2d(src, 2, 1) on an H x W map with a zero
        last row and column; mode 1: max_pool2d(avg_pool2d(src, 2, 1), 3, 2, 1) on H/2 x W/2."""
        assert not src.up and src.f32 == self.f32_mode and src.cmap is None
        if src.H % 2 or src.W % 2 or src.H < 2 or src.W < 2:
            raise NotImplementedError(f"{name}: a {src.H} x {src.W} map (the pooling front end takes even sizes)")
        v = 4 if self.f32_mode else 8
        if src.C % v or src.coff % v:
            raise NotImplementedError(f"{name}: {src.C} channels at offset {src.coff} are not multiples of {v}")
        OH, OW = (src.H // 2, src.W // 2) if mode else (src.H, src.W)
        dst = self.alloc(src.C, OH, OW)
        self._emit(L.OP_POOL_DOWN, name, src0=src, dst=dst, level=mode)
        return dst

    def aconv(self, name: str, x: T, c2: int) -> T:
        """block.py:3692-3703: cv1(avg_pool2d(x, 2, 1, 0, False, True)), cv1 = Conv 3x3 s2 p1.  Over the zero-bordered H x W map the conv
        reads what it reads from the (H-1) x (W-1) pooled map and its padding: an ordinary even-sized stride-2 conv."""
        return self.conv(name + ".cv1", self.pool_down(name + ".pool", x, 0), c2, 3, 2)

    def adown(self, name: str, x: T, c2: int) -> T:
        """block.py:3706-3723: the same average pool, chunk(2, 1); cat(cv1(first half), cv2(max_pool2d(second half, 3, 2, 1))).  The
        halves read disjoint channels: one launch each, the two convs write the halves of one buffer."""
        h, c = x.C // 2, c2 // 2
        if x.C % 2 or c2 % 2 or ((h % 8 or c % 8) and not self.f32_mode):
            raise NotImplementedError(f"{name}: ADown halves of {h} -> {c} channels are not on the fp16 path (multiples of 8)")
        a = self.pool_down(name + ".avg", x.slice(0, h), 0)
        b = self.pool_down(name + ".max", x.slice(h, h), 1)
        out = self.alloc(c2, x.H // 2, x.W // 2)
        self.conv(name + ".cv1", a, c, 3, 2, dst=out.slice(0, c))
        self.conv(name + ".cv2", b, c, 1, 1, dst=out.slice(c, c))
        return out

    def elan(self, name: str, x, c2: int, c3: int, c4: int, n: int, rep: bool) -> T:
        """block.py:3654-3676 RepNCSPELAN4 (rep) / :3679-3689 ELAN1: cv4(cat(y0, y1, cv2(y1), cv3(cv2(y1)))), [y0 | y1] = cv1(x); cv2 / cv3
        are RepCSP -> Conv 3x3 (rep) or one Conv 3x3.  One concat buffer of c3 + 2 c4 channels, every stage a slice of it."""
        xs = [x] if isinstance(x, T) else list(x)
        h = c3 // 2
        if c3 % 2:
            raise NotImplementedError(f"{name}: cv1's {c3} channels do not chunk into two halves")
        # fp16 path, a chunk or branch width that is no multiple of 8 (yolov9m's P4 stage: 360 -> 180 + 180, branches of 180): every piece
        # of the concat is carried on the next multiple of 8 with zero weights and bias in the padding, as c2f / c3k do (T.cmap)
        H, W = xs[0].H, xs[0].W
        cat, h8 = self.pieces([h, h, c4, c4], H, W)
        c8 = self.stored(c4)
        self.conv(name + ".cv1", xs, 2 * h8, 1, 1, dst=cat.slice(0, 2 * h8))
        src = cat.slice(h8, h8)
        for j, cv in enumerate(("cv2", "cv3")):
            dst = cat.slice(2 * h8 + j * c8, c8)
            if rep:
                t = self.pieces([c4], H, W)[0]
                if cat.cmap is not None and t.cmap is None:  # (padded chunks beside a branch width that needs none: the branch's
                    t = t.padded([(c8, c4)])                  # map still says which channels are real, and its weight records with it)
                self.c3k(f"{name}.{cv}.0", src, t, n, True, (3, 3), rep=True)
                self.conv(f"{name}.{cv}.1", t, c8, 3, 1, dst=dst)
            else:
                self.conv(f"{name}.{cv}", src, c8, 3, 1, dst=dst)
            src = dst
        return self.conv(name + ".cv4", cat, c2, 1, 1)

    def c2psa(self, name: str, x: T, c2: int, n: int = 1, psa: bool = False) -> T:
        """block.py:4429-4468 with PSABlock :4348-4383 and Attention :4235-4288.  psa: the PSA module (:4386-4426, YOLOv10) -- the same
        dataflow with exactly one block and no repeat argument, whose `attn`, `ffn.0` and `ffn.1` stand directly under the layer."""
        assert n == 1 or not psa
        assert x.C == c2
        c = int(c2 * 0.5)
        nh = c // 64
        hd = c // nh
        kd = int(hd * 0.5)
        if not self.f32_mode and not kernel_takes("attention", kd, hd):
            # e.g. a width multiple of 0.3125: heads of 40 / 80 channels; the fp32-storage modes run any head shape
            raise NotImplementedError(f"{name}: attention heads of key_dim {kd} / head_dim {hd} are not on the fp16 path (16..64 in steps of 16 / 32..128 in steps of 32)")
        ab = self.alloc(2 * c, x.H, x.W)
        self.conv(name + ".cv1", x, 2 * c, 1, 1, dst=ab)
        b = ab.slice(c, c)
        per = 2 * kd + hd
        perm = qkv_perm(nh, kd, hd)
        for i in range(n):
            pn = name if psa else f"{name}.m.{i}"
            qkv = self.conv(pn + ".attn.qkv", b, nh * per, 1, 1, act=False, perm=perm)
            att = self.alloc(c, x.H, x.W)
            N = x.H * x.W
            attn = dict(src0=qkv, dst=att, heads=nh, key_dim=kd, head_dim=hd, scale=float(kd ** -0.5))
            fl = 2 * self.B * nh * N * N * (kd + hd)
            if self.fuse_attn_pe:  # v@attn^T + pe(v) in one launch: the same weight record and the same bits as the two below
                key = self._wrec(pn + ".attn.pe", name=pn + ".attn.pe", kind="dw", cout=c, cin=1, k=3, real_cout=0)
                self._emit(L.OP_ATTN, pn + ".attn+pe", fl + 2 * self.B * N * c * 9, act=1, wkey=key, **attn)
                xo = att
            else:
                self._emit(L.OP_ATTN, pn + ".attn", fl, **attn)
                xo = self.dwconv(pn + ".attn.pe", qkv.slice(2 * nh * kd, c), act=False, res=att)  # v@attn^T + pe(v)
            self.conv(pn + ".attn.proj", xo, c, 1, 1, act=False, dst=b, res=b)                # b = b + proj(.)
            f = self.conv(pn + ".ffn.0", b, 2 * c, 1, 1)
            self.conv(pn + ".ffn.1", f, c, 1, 1, act=False, dst=b, res=b)                     # b = b + ffn(b)
        return self.conv(name + ".cv2", ab, c2, 1, 1)

    def deconv(self, name: str, x: T, cout: int) -> T:
        """nn.ConvTranspose2d(c1, cout, 2, 2, 0) with bias, no activation (Proto.upsample, block.py:91; YOLOv6's top-level upsamplers):
        out[2i + dy, 2j + dx] = W[:, :, dy, dx]^T x[i, j] + b, so four 1x1 CONV ops, one per output phase (dy, dx), each writing its pixels
        of the double-size map through dst_scale = 2.  One weight record per phase (weights.py kind "deconv"), all read `name`.weight / .bias."""
        assert not x.up
        if not self.f32_mode and (x.C % 8 or x.coff % 8):
            raise NotImplementedError(f"{name}: source channels / offset {(x.C, x.coff)} are not multiples of 8 (fp16 path)")
        up = self.alloc(cout, 2 * x.H, 2 * x.W)
        for dy in (0, 1):
            for dx in (0, 1):
                key = f"{name}@{dy}{dx}"
                if key not in self.wrecs:
                    self.wrecs[key] = WRec(name=name, kind="deconv", cout=cout, cin=x.C, k=1, tap=(dy, dx))
                fl = 2 * self.B * x.H * x.W * cout * x.C
                self._emit(L.OP_CONV, key, fl, src0=x, src1=None, dst=T(up.buf, up.ld, 0, cout, x.H, x.W, False, up.f32), res=None, ksize=1,
                           stride=1, pad=0, act=0, out_f32=0, wkey=key, dst_scale=2, dst_dy=dy, dst_dx=dx, mfma_flops=fl)
        return up

    def proto(self, name: str, x: T, c_: int, nm: int) -> T:
        """block.py:80-97 Proto: cv3(cv2(ConvTranspose2d(c_, c_, 2, 2)(cv1(x)))) -> (B, nm, 2H, 2W)."""
        t = self.conv(name + ".cv1", x, c_, 3, 1)
        up = self.deconv(name + ".upsample", t, c_)
        t = self.conv(name + ".cv2", up, c_, 3, 1)
        p = self.conv(name + ".cv3", t, nm, 1, 1)
        self._emit(L.OP_NHWC2NCHW, name + ".nchw", src0=p, dst=self._ext("proto", self.EXT_PROTO, nm, (p.H, p.W)), OH=0, OW=0, out_dtype=self.out_dtype)
        self.meta.update(proto_hw=(p.H, p.W))
        return p

    def _decoding_conv(self, name: str, src: T, k: int, *, cout: int, mode: int, level: int, a0: int, A: int, nc: int, stride: float,
                       flops: int, **fields):
        """A conv op with the Detect decoder in its epilogue (out_f32 = mode 2: class branch / 3: box branch): it writes level `level`'s
        rows of the prediction tensor (first anchor a0 of A, stride `stride`) and that level's raw map."""
        if mode == 3 and self._e2e:
            mode = 4  # an end2end head's boxes are corners (head.py:148): the box epilogue's xyxy form
        self._emit(L.OP_CONV, name, flops, src0=src, src1=None, dst=self._y(4 + nc, A), res=None, OH=src.H, OW=src.W, ksize=k,
                   stride=1, pad=k // 2, out_f32=mode, dst_scale=1, cout=cout, nl=cout, nc=nc, nm=0, A=A, box=[self._raw(level, nc, src)], cls=[], msk=[], level=level,
                   lvl_h=[src.H, a0], lvl_w=[src.W], lvl_stride=[stride], out_dtype=self.out_dtype, mfma_flops=flops, **fields)

    def _head_conv(self, name: str, src: T, cout: int, mode: int, level: int, a0: int, A: int, nc: int, stride: float, real_cin: int = 0,
                   wrec: Optional[dict] = None):
        """Last 1x1 conv of a Detect branch with the decoder fused into its epilogue (out_f32 = mode 2 / 3).  wrec: fields of the weight
        record that differ from a plain conv's (WorldDetect's folded class conv: kind, post, embed)."""
        key = self._wrec(name, **dict(dict(name=name, kind="plain", cout=cout, cin=src.C, k=1, perm=None, real_cin=real_cin), **(wrec or {})))
        self._decoding_conv(name, src, 1, cout=cout, mode=mode, level=level, a0=a0, A=A, nc=nc, stride=stride,
                            flops=2 * self.B * src.H * src.W * cout * src.C, act=0, wkey=key)

    def _box_tail(self, name: str, i: int, src: T, level: int, a0: int, A: int, nc: int, stride: float, cv2: str = "cv2"):
        """cv2.i.1 (3x3, 64 -> 64, SiLU) + cv2.i.2 (1x1, 64 -> 64 box logits) + DFL / dist2bbox (head.py:49-57, :141-146) as ONE
        conv op: the patch kernel's TAIL form (conv_patch.hip) multiplies its activated fp16 tile with the 1x1 weights straight from
        LDS and decodes the accumulators -- bit for bit what the two launches produce, without the 64-channel map's round trip."""
        n1, n2 = f"{name}.{cv2}.{i}.1", f"{name}.{cv2}.{i}.2"
        k1 = self._wrec(n1, name=n1, kind="conv", cout=64, cin=src.C, k=3, perm=None)
        k2 = self._wrec(n2, name=n2, kind="plain", cout=64, cin=64, k=1, perm=None)
        self._decoding_conv(n1 + "+2", src, 3, cout=64, mode=3, level=level, a0=a0, A=A, nc=nc, stride=stride,
                            flops=2 * self.B * src.H * src.W * 64 * (9 * src.C + 64), act=self.act_id, wkey=k1, wkey2=k2, mid_c=64)

    def detect(self, name: str, xs: List[T], nc: int, legacy: bool, nm: int = 0, npr: int = 0, ne: int = 0, nk: int = 0, kdim: int = 0,
               end2end: bool = False, world: Optional[Tuple[int, int]] = None):
        """head.py:21-148 (+ Segment :175-197, OBB :200-227 with ne angle channels, Pose :230-279 with nk = nkpt * kdim keypoint
        channels).  end2end: v10Detect (:592-625, forward_end2end :76-98) -- the one2one copy of the branches (one2one_cv2 / one2one_cv3)
        decodes corner boxes into the pre-top-k tensor `pre` and writes the one2one raw maps `o2o{l}`, BSY_OP_E2E_TOPK turns `pre` into the
        rows (B, min(max_det, A), 6); the one2many copy (cv2 / cv3: raw maps `o2m{l}` only, nothing decoded) is emitted in a plan built
        with one2many=True alone, always through f32 logit maps and the raw-map transposes (the fused epilogues write a prediction tensor).
        world = (embed, the yaml's nc): WorldDetect with the BatchNorm contrastive head (head.py:307-320, block.py:3609-3631) -- `nc` is then the
        number of text rows scored, the hidden width c3 comes from the yaml's nc as the constructor computed it (head.py:313), and the last
        class conv of every level is cv4.l folded into cv3.l.2 (weights.py kind "world_cls"): BatchNorm, the dot products with the unit text
        rows, exp(logit_scale) and the bias are all linear in the embedding, itself a biased 1x1 conv.  The legacy Detect lowering otherwise."""
        if end2end:
            assert not (nm or ne or nk or legacy)
            start = len(self.ops)
            self._e2e = "o2o"
            self._detect(name, xs, nc, False, 0, 0, 0, 0, "one2one_")
            if self.one2many:
                self._e2e = "o2m"
                self._detect(name, xs, nc, False, 0, 0, 0, 0, "")
            self._e2e = "o2o"
            # every branch chain of both copies first, each on its lane; then what runs on lane 0 behind a join: the decode launch (a
            # plan without the fused head), the top-k, and last the raw-map transposes, which nothing waits for
            head = self.ops[start:]
            self.ops[start:] = ([o for o in head if o["kind"] not in (L.OP_DECODE, L.OP_RAW_NCHW)] + [o for o in head if o["kind"] == L.OP_DECODE])
            A, K = self.meta["A"], min(self.max_det, self.meta["A"])
            self.buf_bytes.append(int(L.lib.bsy_end2end_topk_workspace_bytes(self.B, A, nc, self.max_det)))
            scratch = T(len(self.buf_bytes) - 1, 0, 0, 0, 1, 1, False, True)
            self._emit(L.OP_E2E_TOPK, name + ".topk", join=1, src0=self._y(4 + nc, A), res=scratch, nc=nc, A=A, ksize=self.max_det, H=self.H,
                       W=self.W, OH=0, OW=0, dst=self._ext("rows", self.EXT_ROWS, K, (6,), dtype="float32"), out_dtype=self.out_dtype)
            self.ops += [o for o in head if o["kind"] == L.OP_RAW_NCHW]
            self._e2e = ""
            self.meta.update(end2end=True, max_det=self.max_det, K=K, one2many=self.one2many)
            return
        self._detect(name, xs, nc, legacy, nm, ne, nk, kdim, "", world)

    def _detect(self, name: str, xs: List[T], nc: int, legacy: bool, nm: int, ne: int, nk: int, kdim: int, pfx: str,
                world: Optional[Tuple[int, int]] = None):
        """One copy of the head's branches: `pfx` in front of cv2 / cv3 ("one2one_" for v10Detect's one2one copy)."""
        cv2, cv3 = f"{name}.{pfx}cv2", f"{name}.{pfx}cv3"
        o2m = self._e2e == "o2m"
        lane0 = 2 * len(xs) if o2m else 0  # (an end2end head has no cv4 branches: their lanes carry the one2many copy)
        if not 1 <= len(xs) <= L.BSY_MAX_LEVELS:
            raise NotImplementedError(f"{name}: a head on {len(xs)} levels (1 to {L.BSY_MAX_LEVELS} are accelerated)")
        if ne and len(xs) > 3:
            raise NotImplementedError(f"{name}: an OBB head on {len(xs)} levels (the reference ships none) is not accelerated")
        ch = [t.C for t in xs]
        c2, c3 = max(16, ch[0] // 4, 64), max(ch[0], min(world[1] if world else nc, 100))
        boxes, clss, msks = [], [], []
        A = sum(t.H * t.W for t in xs)
        a0 = [sum(t.H * t.W for t in xs[:i]) for i in range(len(xs))]
        strides = [float(self.H // t.H) for t in xs]
        # Detect without mask coefficients: the last conv of every branch decodes in its epilogue (conv_kernels.h
        # conv_epilogue_head) -- no f32 logit maps, no decode launch, no raw-map transposes.  An OBB head's box decode needs the
        # angle of its cv4 branch (tal.py:404-423 dist2rbox), so OBB always takes the decode launch
        # Four levels (P2 / P6 graphs) fuse the same way: every fused op carries its own level, first anchor and stride
        # A Pose head takes the decode launch too: it decodes the keypoint rows there (csrc/detect.hip, mode DEC_KPT)
        fused = self.fuse_head and nm == 0 and ne == 0 and nk == 0 and not o2m
        # every (level, branch) chain is independent until the decoder: give each its own lane so the engine runs them
        # concurrently (the 40x40 / 20x20 chains are far too small to fill 256 CUs on their own)
        for i, x in enumerate(xs):
            assert not x.up
            self._lane = lane0 + 2 * i
            t = self.conv(f"{cv2}.{i}.0", x, c2, 3, 1)
            if fused and self.fuse_boxtail and c2 == 64:
                self._box_tail(name, i, t, i, a0[i], A, nc, strides[i], pfx + "cv2")
            else:
                t = self.conv(f"{cv2}.{i}.1", t, c2, 3, 1)
                if fused:
                    self._head_conv(f"{cv2}.{i}.2", t, 64, 3, i, a0[i], A, nc, strides[i])
                else:
                    boxes.append(self.conv(f"{cv2}.{i}.2", t, 64, 1, 1, act=False, plain=True, out_f32=True))
            self._lane = lane0 + 2 * i + 1
            # c3 = max(ch0, min(nc, 100)) (head.py:39) need not be a multiple of 8 (YOLO11n with 65 .. 100 or more classes: 100): the
            # branch then runs c3p channels wide with zero weights / biases in the padding -- SiLU(0) = 0 all the way, same results
            c3p = make_divisible(c3, 8)
            r3 = c3 if c3p != c3 else 0
            if legacy:
                t = self.conv(f"{cv3}.{i}.0", x, c3p, 3, 1, real=(r3, 0))
                t = self.conv(f"{cv3}.{i}.1", t, c3p, 3, 1, real=(r3, r3))
            else:
                t = self.dwpw(f"{cv3}.{i}.0", x, c3p, real=(r3, 0))
                t = self.dwpw(f"{cv3}.{i}.1", t, c3p, real=(r3, r3))
            if fused:
                self._head_conv(f"{cv3}.{i}.2", t, nc, 2, i, a0[i], A, nc, strides[i], real_cin=r3,
                                wrec=dict(kind="world_cls", post=f"{name}.cv4.{i}", embed=world[0]) if world else None)
            else:
                clss.append(self.conv(f"{cv3}.{i}.2", t, nc, 1, 1, act=False, plain=True, out_f32=True, real=(0, r3), wkind="world_cls" if world else None))
                if world:
                    r = self.wrecs[f"{cv3}.{i}.2"]
                    r.post, r.embed = f"{name}.cv4.{i}", world[0]
            if nm or ne:
                # Segment.cv4 (head.py:175-197) / OBB.cv4 (:208-209): Conv(x, c4, 3) -> Conv(c4, c4, 3) -> Conv2d(c4, nm or ne, 1), on lanes
                # of their own.  OBB's angle logits land in an f32 map 8 channels wide (zero weights and bias past `ne`): the conv kernels
                # write cout in 8-channel pieces and the decoder reads 16-byte rows; it passes them in the msk slots with nm = 0
                self._lane = 2 * len(xs) + i
                c4 = max(ch[0] // 4, nm or ne)
                wout, real = (nm, 0) if nm else (make_divisible(ne, 8), ne)
                t = self.conv(f"{name}.cv4.{i}.0", x, c4, 3, 1)
                t = self.conv(f"{name}.cv4.{i}.1", t, c4, 3, 1)
                msks.append(self.conv(f"{name}.cv4.{i}.2", t, wout, 1, 1, act=False, plain=True, out_f32=True, real=(real, 0)))
            elif nk:
                # Pose.cv4 (head.py:239-240), the same shape of branch on the same lanes.  c4 = max(ch0 // 4, nk) is 51 for every stock
                # n / s model: like the class branch's c3, the branch then runs on the next multiple of 8 with zero weights and biases
                # in the padding.  The keypoint logits land in an f32 map make_divisible(nk, 8) wide, as OBB's angle does
                self._lane = 2 * len(xs) + i
                c4 = max(ch[0] // 4, nk)
                c4p, wout = make_divisible(c4, 8), make_divisible(nk, 8)
                r4 = c4 if c4p != c4 else 0
                t = self.conv(f"{name}.cv4.{i}.0", x, c4p, 3, 1, real=(r4, 0))
                t = self.conv(f"{name}.cv4.{i}.1", t, c4p, 3, 1, real=(r4, r4))
                msks.append(self.conv(f"{name}.cv4.{i}.2", t, wout, 1, 1, act=False, plain=True, out_f32=True,
                                      real=(nk if wout != nk else 0, r4)))
        self._lane = 0
        self.meta.update(A=A, nc=nc, nm=nm, ne=ne, no=64 + nc, strides=strides, levels=[(t.H, t.W) for t in xs])
        if fused:
            return
        # a Detect head that takes the decode launch on the fp16 path does so because fuse_head is off: the launch then sums the DFL in
        # the fused epilogue's order (act = 1), so the switch returns the fused plan's bits at three levels as it does at four.  Segment,
        # OBB and the fp32-storage modes have no fused form and keep the order their outputs have always had
        lvl = dict(H=self.H, W=self.W, OH=0, OW=0, nl=len(xs), nc=nc, A=A, box=boxes, cls=clss, lvl_h=[t.H for t in xs], lvl_w=[t.W for t in xs],
                   lvl_stride=strides, out_dtype=self.out_dtype)
        kraw = self._ext("kpt", self.EXT_KPT, nk, (A,), raw_only=True) if nk else None
        if not o2m:  # (act: bit 0 = the fused epilogue's DFL order, bit 1 = corner boxes, an end2end head's)
            self._emit(L.OP_DECODE, name + ".decode", join=1, nm=nm, ne=ne, nk=nk, kdim=kdim, msk=msks, res=kraw,
                       act=int(not self.f32_mode and nm == 0 and ne == 0 and nk == 0) | (2 if self._e2e else 0),
                       dst=self._y(4 + nc + nm + ne + nk, A), **lvl)
        for i, x in enumerate(xs):
            self._emit(L.OP_RAW_NCHW, f"{name}.{self._e2e or 'raw'}{i}", nm=0, msk=[], level=i, dst=self._raw(i, nc, x), **lvl)

    def classify(self, name: str, x: T, nc: int):
        """head.py:282-304 Classify in eval: (y, x) = (softmax(x), x), x = linear(pool(conv(x)).flatten(1)); Dropout(p = 0) is the
        identity.  conv is an ordinary 1x1 Conv (BN folded, SiLU); the global mean is OP_GAP; linear is a plain 1x1 conv on the
        (B, 1, 1, 1280) map writing f32 logits (a class count that is no multiple of 8 on the next one, zero weights and bias in the
        padding, as the OBB angle branch does); OP_CLASSIFY_TAIL turns the logits into y, x and the top-k rows (csrc/classify.hip)."""
        assert not x.up
        t = self.conv(name + ".conv", x, 1280, 1, 1)
        g = self.alloc(1280, 1, 1)
        self._emit(L.OP_GAP, name + ".pool", src0=t, dst=g)
        ncp = make_divisible(nc, 8)
        lg = self.conv(name + ".linear", g, ncp, 1, 1, act=False, plain=True, out_f32=True, real=(nc if ncp != nc else 0, 0))
        k = min(nc, 5)  # what the predictor and the validator rank (classify/predict.py:51-60, val.py:56-60)
        idx, val = self._ext("topk_idx", self.EXT_TOPK_IDX, k, dtype="int32"), self._ext("topk_val", self.EXT_TOPK_VAL, k, dtype="float32")
        self._emit(L.OP_CLASSIFY_TAIL, name + ".tail", src0=lg, dst=self._ext("y", self.EXT_Y, nc), res=self._ext("x", self.EXT_LOGITS, nc, raw_only=True),
                   nc=nc, ksize=k, box=[idx], cls=[val], out_dtype=self.out_dtype, OH=0, OW=0)
        # strides: the engine's size multiple (the backbone halves the map five times); ClassificationModel.stride itself is 1
        # (tasks.py:457).  No anchors, levels or raw maps: the engine's readers of A / levels / no see an empty head
        self.meta.update(task="classify", nc=nc, nm=0, ne=0, A=0, no=0, strides=[32.0], levels=[], topk=k)
        self.pooled = g  # the (B, 1, 1, 1280) mean, for tests that read it back (YoloEngine.read_view)

    # ---- graph walk (nn/tasks.py:138-165 + :940-1105) -----------------------------------------------------------
    # A graph under `activation: nn.ReLU()`: the modules it may hold, and the op kinds they may lower to -- the four whose `act` is an
    # activation id, and the glue (copies, pools, the decode launch and the raw-map transposes), which applies none
    RELU_MODULES = ("Conv", "SPPF", "nn.ConvTranspose2d", "nn.Upsample", "nn.MaxPool2d", "nn.ZeroPad2d", "Concat", "Detect")
    RELU_KINDS = (L.OP_CONV_FIRST, L.OP_FIRST_POOL, L.OP_STEM, L.OP_CONV, L.OP_COPY, L.OP_S2D, L.OP_SPPF_POOL, L.OP_MAXPOOL, L.OP_DECODE, L.OP_RAW_NCHW)

    # Modules that are refused with a reason of their own (everything else outside LOWERINGS: "not on the accelerated path")
    REFUSED = {"ImagePoolingAttn": "YOLO-World v1 (yolov8-world.yaml) updates the text features per image from the feature maps; v2 "
                                   "(yolov8-worldv2.yaml), whose text features are constant per call, is the accelerated graph"}

    def _build(self):
        """The bookkeeping every layer shares; what a module lowers to is its entry of LOWERINGS below."""
        d = self.cfg
        depth, self.width, self.max_ch, self.scale = d.get("depth_multiple", 1.0), d.get("width_multiple", 1.0), float("inf"), d.get("scale")
        if d.get("scales"):
            if not self.scale:
                self.scale = next(iter(d["scales"]))
            depth, self.width, self.max_ch = d["scales"][self.scale]
        nc, relu = d["nc"], self.act_id == L.ACT_RELU
        if self.text_nc is not None and (list(d["head"]) or [[0, 0, ""]])[-1][2] != "WorldDetect":
            raise ValueError("text_nc is read by a graph under a WorldDetect head alone")
        self.legacy = True  # Detect's class branch is the heavy one (head.py:44-56) until a C3k2 says otherwise (tasks.py:1048)
        self.layers = layers = list(d["backbone"]) + list(d["head"])
        outs: List = []   # per layer: T, or list[T] for a lazy Concat
        self._first_layer = 0  # the layer that emits op 0, the first reader of the image: 0, or 1 behind an accepted nn.Identity
        x, ly, last, lowerings = None, _Layer(), len(layers) - 1, self.LOWERINGS
        for i, (f, n, m, args) in enumerate(layers):
            name = f"model.{i}"
            args = [nc if a == "nc" else a for a in args]
            if f != -1:
                x = outs[f] if isinstance(f, int) else [x if j == -1 else outs[j] for j in f]
            if isinstance(x, _ZeroPadded):
                x.gate(i, m)
            if m != "CBFuse":
                for t in x if isinstance(x, list) else [x]:
                    if isinstance(t, _Slices):
                        raise NotImplementedError(f"{name}: {m} reads the output of CBLinear model.{t.layer}: its channel groups are views that "
                                                  "only a CBFuse may read")
            if relu and m not in self.RELU_MODULES:
                # ReLU exists in the kernels of CONV_FIRST / FIRST_POOL / STEM / CONV alone; every block module lowers to other kinds as
                # well (and, in this fork, would keep SiLU anyway: block.py:13 shadows Conv there).  No silent SiLU where the reference
                # may hold ReLU, or the reverse: the graph stays on the reference
                raise NotImplementedError(f"{name}: {m} under activation nn.ReLU() is not accelerated (ReLU graphs: {', '.join(self.RELU_MODULES)})")
            lower, scaled = lowerings.get(m, (None, False))
            if lower is None:
                if m in self.REFUSED:
                    raise NotImplementedError(f"{name}: {m} is not accelerated: {self.REFUSED[m]}")
                raise NotImplementedError(f"module {m} is not on the accelerated path")
            first_op = len(self.ops)
            ly.i, ly.name, ly.m, ly.x, ly.args, ly.n, ly.last = i, name, m, x, args, max(round(n * depth), 1) if n > 1 else n, i == last
            ly.c2 = self._scaled(args[0]) if scaled else None
            x = lower(self, ly)
            if first_op == 0 and self.ops:
                self._first_layer = i
            if relu:  # what RELU_MODULES promises, checked on the ops themselves
                for o in self.ops[first_op:]:
                    if o["kind"] not in self.RELU_KINDS:
                        raise NotImplementedError(f"{name}: {m} lowers to op {o['name']} of kind {o['kind']}, which has no ReLU (activation nn.ReLU())")
            outs.append(x)
        self.layer_out = [t if isinstance(t, (T, list)) else None for t in outs]  # (a _ZeroPadded, a _Slices, the image, a head: no map)
        self.meta.update(scale=self.scale, n_layers=len(layers), legacy=self.legacy)
        self._fuse_stem()
        self._fuse_first_pool()

    def _scaled(self, c: int) -> int:  # parse_model's width scaling of a channel count (tasks.py:1016)
        return make_divisible(min(c, self.max_ch) * self.width, 8)

    # ---- lowerings (LOWERINGS below): ly is the layer's _Layer, the result the layer's output -- a T, a list of T (a lazy Concat), a
    # _ZeroPadded, or None (a head).  A module's arguments are [c2, ...] as the yaml has them; ly.c2 is the first one width-scaled
    def _m_conv(self, ly: _Layer):
        name, x, n, c2, k, s = ly.name, ly.x, ly.n, ly.c2, ly.arg(1, 1), ly.arg(2, 1)
        pad = k // 2 if ly.arg(3, None) is None else ly.args[3]
        if x is None:  # the image: layer 0, or a layer that reads an accepted nn.Identity at layer 0 (yolov9e's layers 1 and 15)
            if n > 1:
                raise NotImplementedError(f"{name}: an image conv repeated {n} times is not accelerated")
            if (k, s, pad) not in ((3, 2, 1), (3, 1, 1), (6, 2, 2)):
                raise NotImplementedError(f"image conv k={k} s={s} p={pad}: 3x3 s2 p1, 3x3 s1 p1 or 6x6 s2 p2 only")
            return self.conv_first(name, c2, k, s, pad)
        # n > 1: parse_model's nn.Sequential of n Convs (tasks.py:1094), every one built Conv(c1, c2, k, s): model.i.0 .. model.i.{n-1}
        # (YOLOv6's equal-width 3x3 chains).  From the second on a link reads c2 channels, so the chain exists where c1 == c2
        if n > 1 and (not isinstance(x, T) or x.C != c2):
            raise NotImplementedError(f"{name}: {n} chained Convs need an input of their own width ({c2} channels)")
        assert n > 1 or isinstance(x, T) or all(isinstance(t, T) for t in x)  # (a list: a two-operand Concat, yolov3-tiny's layer 19)
        if pad != k // 2:
            raise NotImplementedError(f"Conv with padding {pad} != k // 2 is not accelerated")
        if n > 1:
            for j in range(n):
                x = self.conv(f"{name}.{j}", x, c2, k, s)
            return x
        return self.conv(name, x, c2, k, s)

    def _m_c3(self, ly: _Layer):  # C3 (block.py:3320-3334), C3Ghost (:3374-3381); parse_model inserts the repeat count (tasks.py:1033, :1038)
        y, ghost = self.alloc_like(ly.x, ly.c2), ly.m == "C3Ghost"
        self.c3k(ly.name, ly.x, y, ly.n, ghost or bool(ly.arg(1, True)), k=(3, 3) if ghost else (1, 3), ghost=ghost)
        return y

    def _m_ghostconv(self, ly: _Layer):  # conv.py:280-293, args [c2, k, s, g, act]; the yamls' stride-2 3x3 downsamplers
        if ly.x is None or ly.arg(3, 1) != 1:
            raise NotImplementedError(f"{ly.name}: GhostConv on the image or with g = {ly.arg(3, 1)} is not accelerated")
        self._fp16_mult8(ly.c2 // 2, f"{ly.name}: a top-level GhostConv with halves of {ly.c2 // 2} channels is not on the fp16 path (multiples of 8)")
        return self.ghostconv(ly.name, ly.x, ly.c2, ly.arg(1, 1), ly.arg(2, 1), bool(ly.arg(4, True)))

    def _m_ghost_bottleneck(self, ly: _Layer):  # block.py:3384-3402, args [c2, k, s]
        assert isinstance(ly.x, T)
        y = self.alloc_like(ly.x, ly.c2)
        self.ghost_bottleneck(ly.name, ly.x, y, ly.arg(2, 1))
        return y

    def _m_dwconv(self, ly: _Layer):  # conv.py:224-229: Conv(c1, c2, k, s, g=gcd(c1, c2))
        x, k, s = ly.x, ly.arg(1, 1), ly.arg(2, 1)
        assert isinstance(x, T)
        if ly.c2 != x.C:
            raise NotImplementedError(f"DWConv {x.C} -> {ly.c2}: only the depthwise case c1 == c2 is accelerated")
        return self.dwconv_g(ly.name, x, k, k, s, x.C)

    def _m_c3k2(self, ly: _Layer):  # C3k2, and C3k2_gai (tasks.py:1038: the repeat count inserted, no m/l/x override, `legacy` untouched)
        c3k, gai = bool(ly.arg(1, False)), ly.m == "C3k2_gai"
        if not gai:
            self.legacy = False
            c3k = bool(self.scale and self.scale in "mlx") or c3k  # (tasks.py:1046-1049)
        return self.c2f(ly.name, ly.x, ly.c2, ly.n, True, ly.arg(2, 0.5), ("c3k_gai" if c3k else "pmsfa") if gai else ("c3k" if c3k else "bottleneck"))

    def _m_c2f(self, ly: _Layer):  # C2f [c2, shortcut]; C2fCIB (block.py:4215-4232) [c2, shortcut, lk]; repeat count inserted (tasks.py:1037-1043)
        cib = ly.m == "C2fCIB"
        return self.c2f(ly.name, ly.x, ly.c2, ly.n, bool(ly.arg(1, False)), 0.5, "cib" if cib else "c2f", lk=cib and bool(ly.arg(2, False)))

    def _m_c2fattn(self, ly: _Layer):
        """C2fAttn [c2, ec, nh] (block.py:3518-3535); parse_model scales ec and nh (tasks.py:1017-1021) and inserts the repeat count.  Its
        guide is the text the head scores, so it stands in a graph under WorldDetect alone."""
        if self.layers[-1][2] != "WorldDetect":
            raise NotImplementedError(f"{ly.name}: C2fAttn in a graph whose head is {self.layers[-1][2]}, not WorldDetect (the text features "
                                      "that guide it come with that head) is not accelerated")
        inf = float("inf")
        half = inf if self.max_ch == inf else self.max_ch // 2
        ec = make_divisible(min(ly.args[1], half) * self.width, 8)
        nh = ly.arg(2, 1)
        if nh > 1:
            nh = int(max(round(min(nh, inf if half == inf else half // 32)) * self.width, 1))
        return self.c2f_attn(ly.name, ly.x, ly.c2, ly.n, ec, nh)

    def _m_c2(self, ly: _Layer):  # the necks of yolov8-p6.yaml / yolov8-seg-p6.yaml
        return self.c2(ly.name, ly.x, ly.c2, ly.n, bool(ly.arg(1, True)))

    def _m_scdown(self, ly: _Layer):
        assert isinstance(ly.x, T)
        return self.scdown(ly.name, ly.x, ly.c2, ly.args[1], ly.args[2])

    def _m_c2psa(self, ly: _Layer):  # C2PSA; PSA (block.py:4386-4426), args [c2]: no repeat count (tasks.py:1010), one block
        assert isinstance(ly.x, T)
        return self.c2psa(ly.name, ly.x, ly.c2, 1 if ly.m == "PSA" else ly.n, psa=ly.m == "PSA")

    def _m_spp(self, ly: _Layer):
        """SPPF; SPP (block.py:3088-3111, args [c2, k]): cv2(cat(x', m5 x', m9 x', m13 x')), x' = cv1(x) -- stride-1 max pools compose, m5 . m5
        = m9, m5 . m5 . m5 = m13, bit for bit, so k = (5, 9, 13) is SPPF's dataflow under the same names; SPPELAN (args [c2, c3, k])."""
        m, name, x = ly.m, ly.name, ly.x
        if m == "SPPF":
            assert isinstance(x, T) and ly.arg(1, 5) == 5
        elif m == "SPP":
            if not isinstance(x, T) or list(ly.arg(1, (5, 9, 13))) != [5, 9, 13]:
                raise NotImplementedError(f"{name}: SPP with k = {ly.arg(1, None)} (k = [5, 9, 13] on one input is accelerated)")
            self._fp16_mult8(x.C // 2, f"{name}: SPP with a hidden width of {x.C // 2} channels is not on the fp16 path (multiples of 8)")
        else:
            assert isinstance(x, T)
            if ly.arg(2, 5) != 5:
                raise NotImplementedError(f"{name}: SPPELAN with k = {ly.args[2]} (the pool kernel is built for 5)")
            self._fp16_mult8(ly.args[1], f"{name}: SPPELAN with a hidden width of {ly.args[1]} channels is not on the fp16 path (multiples of 8)")
            return self.sppf(name, x, ly.c2, ly.args[1], "cv5")
        return self.sppf(name, x, ly.c2)

    def _m_bottleneck(self, ly: _Layer):  # block.py:3405-3419, args [c2, shortcut, g, k, e]; n > 1: parse_model's nn.Sequential (tasks.py:1094)
        name, x, n, c2 = ly.name, ly.x, ly.n, ly.c2
        if ly.arg(2, 1) != 1:
            raise NotImplementedError(f"{name}: Bottleneck with g = {ly.args[2]} is not accelerated")
        if n > 1 and (not isinstance(x, T) or x.C != c2):
            raise NotImplementedError(f"{name}: {n} chained Bottlenecks need an input of their own width ({c2} channels)")
        for j in range(n):
            x = self.top_bottleneck(name if n == 1 else f"{name}.{j}", x, c2, bool(ly.arg(1, True)), tuple(ly.arg(3, (3, 3))), ly.arg(4, 0.5))
        return x

    def _m_elan(self, ly: _Layer):  # YOLOv9's modules (tasks.py:995-1023): the arguments behind c2 literal, no repeat count inserted (n stays 1)
        rep = ly.m == "RepNCSPELAN4"  # (else ELAN1)
        return self.elan(ly.name, ly.x, ly.c2, ly.args[1], ly.args[2], ly.arg(3, 1) if rep else 0, rep)

    def _m_down(self, ly: _Layer):
        assert isinstance(ly.x, T)
        return self.aconv(ly.name, ly.x, ly.c2) if ly.m == "AConv" else self.adown(ly.name, ly.x, ly.c2)

    def _m_attention(self, ly: _Layer):  # MSCAAttention (tasks.py:1052-1054), ELA (:1066-1070): built on the input's channels
        assert isinstance(ly.x, T)
        return self.msca(ly.name, ly.x) if ly.m == "MSCAAttention" else self.ela(ly.name, ly.x)

    def _m_zeropad(self, ly: _Layer):
        """Accepted in one place: [[0, 1, 0, 1]] in front of nn.MaxPool2d [2, 1, 0] that reads it alone (yolov3-tiny's layers 11 + 12);
        the pair is one MAXPOOL of mode 1, emitted at the pool."""
        i, name, nxt = ly.i, ly.name, None if ly.last else self.layers[ly.i + 1]
        if not isinstance(ly.x, T) or [list(a) if isinstance(a, (list, tuple)) else a for a in ly.args] != [[0, 1, 0, 1]]:
            raise NotImplementedError(f"{name}: nn.ZeroPad2d {ly.args} (only [[0, 1, 0, 1]] on one input is accelerated)")
        if nxt is None or nxt[0] != -1 or nxt[2] != "nn.MaxPool2d" or list(nxt[3]) != [2, 1, 0]:
            raise NotImplementedError(f"{name}: nn.ZeroPad2d is accelerated only in front of nn.MaxPool2d [2, 1, 0] reading it alone")
        for j, (fj, _, _, _) in enumerate(self.layers):
            if j != i + 1 and any((v if v >= 0 else j + v) == i for v in ([fj] if isinstance(fj, int) else fj)):
                raise NotImplementedError(f"{name}: the output of nn.ZeroPad2d is read by model.{j} as well: the padded map is never stored")
        return _ZeroPadded(ly.x)

    def _m_maxpool(self, ly: _Layer):
        x, ksp = ly.x, (ly.arg(0, None), ly.arg(1, None), ly.arg(2, 0))
        if isinstance(x, _ZeroPadded):
            assert ksp == (2, 1, 0)
            return self.maxpool(ly.name, x.src, 1)
        if isinstance(x, T) and ksp == (2, 2, 0) and len(ly.args) <= 3:
            return self.maxpool(ly.name, x, 0)
        raise NotImplementedError(f"{ly.name}: nn.MaxPool2d {ly.args} (only [2, 2, 0], and [2, 1, 0] behind nn.ZeroPad2d [[0, 1, 0, 1]], are accelerated)")

    def _m_deconv(self, ly: _Layer):
        """args [c2, k, s, p, output_padding, groups, bias, dilation]; the class is in parse_model's base-module set (tasks.py:1006), so c2 is
        width-scaled like a Conv's and c1 put in front -- here behind the refusals, which read no c2.  The 2x2 stride-2 upsampler is accelerated."""
        name, x, arg = ly.name, ly.x, ly.arg
        if not isinstance(x, T) or x.up:
            raise NotImplementedError(f"{name}: nn.ConvTranspose2d on a Concat or an upsampled view is not accelerated")
        if (arg(1, 1), arg(2, 1), arg(3, 0), arg(4, 0), arg(5, 1), arg(6, True), arg(7, 1)) != (2, 2, 0, 0, 1, True, 1) or len(ly.args) > 8 or ly.n != 1:
            raise NotImplementedError(f"{name}: nn.ConvTranspose2d {ly.args} (kernel 2, stride 2, padding 0, no output padding, one group, "
                                      "with bias, once, is accelerated)")
        return self.deconv(name, x, self._scaled(ly.args[0]))

    def _m_identity(self, ly: _Layer):
        """nn.Identity at layer 0 names the image so that a second backbone can read it (yolov9e.yaml: layer 15 reads layer 0).  Its output is
        the image itself (None, as layer 0's input is); accepted only where some layer reads layer 0 by its index -- behind an Identity that
        layer 1 alone reads, every index of a checkpoint's graph is shifted by one for nothing, and the graph stays on the reference."""
        if ly.i != 0:
            raise NotImplementedError(f"{ly.name}: nn.Identity is accelerated as layer 0 (a name for the image) only")
        readers = [j for j, (fj, _, _, _) in enumerate(self.layers) if j and 0 in ([fj] if isinstance(fj, int) else list(fj))]
        if not readers:
            raise NotImplementedError(f"{ly.name}: nn.Identity that no layer reads by index (model.1 alone reads it) is not accelerated")
        for j in sorted(set(readers + [1])):
            fj, _, mj, _ = self.layers[j]
            if (j in readers or fj == -1) and (mj != "Conv" or not isinstance(fj, int)):
                raise NotImplementedError(f"{ly.name}: the image behind nn.Identity is read by model.{j} ({mj}); only a Conv of its own may")
        return None

    def _m_cblinear(self, ly: _Layer):
        """CBLinear [c2s, k, s, p, g] (block.py:3740-3757; tasks.py: c1 = ch[f], the widths literal): a biased nn.Conv2d without BN or
        activation whose output is split into groups of c2s channels.  k = 1: one plain 1x1 CONV into a sum(c2s)-wide buffer; the layer's
        output is the groups as views of it (_Slices)."""
        name, x, arg = ly.name, ly.x, ly.arg
        c2s = arg(0, None)
        if not isinstance(c2s, (list, tuple)) or not c2s or any(not isinstance(c, int) or c < 1 for c in c2s):
            raise NotImplementedError(f"{name}: CBLinear with the widths {c2s!r} (a list of channel counts is accelerated)")
        if (arg(1, 1), arg(2, 1), arg(3, None), arg(4, 1)) != (1, 1, None, 1) or ly.n != 1:
            raise NotImplementedError(f"{name}: CBLinear with k, s, p, g = {ly.args[1:5]} (the default 1x1 conv, once, is accelerated)")
        if not isinstance(x, T) or x.up or x.cmap is not None:
            raise NotImplementedError(f"{name}: CBLinear on a Concat, an upsampled view or zero-padded pieces is not accelerated")
        for c in c2s:
            self._fp16_mult8(c, f"{name}: CBLinear with a group of {c} channels is not on the fp16 path (multiples of 8)")
        y = self.conv(name + ".conv", x, sum(c2s), 1, 1, act=False, plain=True)
        parts, c0 = [], 0
        for c in c2s:
            parts.append(y.slice(c0, c))
            c0 += c
        return _Slices(parts, ly.i)

    def _m_cbfuse(self, ly: _Layer):
        """CBFuse [idx] (block.py:3760-3772): the last input plus group idx[i] of the i-th CBLinear, nearest-upsampled to the last input's
        size -- one OP_CBFUSE into a fresh map (csrc/cbfuse.hip; the sum's order is the reference's: the taps in order, then the last)."""
        name, x = ly.name, ly.x
        idx = ly.arg(0, None)
        if not isinstance(x, list) or len(x) < 2 or not all(isinstance(t, _Slices) for t in x[:-1]):
            raise NotImplementedError(f"{name}: CBFuse reads CBLinear outputs and, last, one map; its inputs are {self.layers[ly.i][0]}")
        last = x[-1]
        if not isinstance(last, T) or last.up or last.cmap is not None:
            raise NotImplementedError(f"{name}: the last input of CBFuse must be a plain map (not a CBLinear output, a Concat, an upsampled "
                                      "view or zero-padded pieces)")
        if not isinstance(idx, (list, tuple)) or len(idx) != len(x) - 1:
            raise NotImplementedError(f"{name}: CBFuse with idx = {idx!r} for {len(x) - 1} CBLinear inputs (one index each)")
        if len(idx) > L.BSY_CBFUSE_MAX_TAPS:
            raise NotImplementedError(f"{name}: CBFuse of {len(idx)} CBLinear inputs (up to {L.BSY_CBFUSE_MAX_TAPS} are accelerated)")
        taps, shifts = [], []
        for s, j in zip(x[:-1], idx):
            if not isinstance(j, int) or not 0 <= j < len(s.parts):
                raise NotImplementedError(f"{name}: idx {j!r} is out of range for CBLinear model.{s.layer} ({len(s.parts)} groups)")
            t = s.parts[j]
            if t.C != last.C:
                raise NotImplementedError(f"{name}: group {j} of CBLinear model.{s.layer} has {t.C} channels, the last input {last.C}")
            k = next((k for k in range(5) if (t.H << k, t.W << k) == (last.H, last.W)), None)
            if k is None:
                raise NotImplementedError(f"{name}: CBLinear model.{s.layer} is {t.H} x {t.W}, the target {last.H} x {last.W}: a tap is "
                                          "upsampled by 1, 2, 4, 8 or 16 (never down)")
            taps.append(t)
            shifts.append(k)
        dst = self.alloc(last.C, last.H, last.W)
        self._emit(L.OP_CBFUSE, name, src0=last, dst=dst, nl=len(taps), box=taps[:L.BSY_MAX_LEVELS], cls=taps[L.BSY_MAX_LEVELS:],
                   lvl_h=shifts[:L.BSY_MAX_LEVELS], lvl_w=shifts[L.BSY_MAX_LEVELS:])
        return dst

    def _m_upsample(self, ly: _Layer):
        x = ly.x
        assert isinstance(x, T) and not x.up and ly.args[1] == 2 and ly.args[2] == "nearest"
        return T(x.buf, x.ld, x.coff, x.C, x.H * 2, x.W * 2, True, x.f32)

    def _m_concat(self, ly: _Layer):
        x = ly.x
        assert isinstance(x, list) and len(x) == 2, "only two-operand Concat feeding a conv is accelerated"
        for j, t in enumerate(x):  # an operand that is itself a (lazy) Concat -- BS-YOLO's layer 21 reads layer 13 -- is materialised once
            if isinstance(t, list):
                assert all(isinstance(u, T) for u in t)
                real = self.alloc_like(t, sum(u.C for u in t))
                c0 = 0
                for u in t:
                    self.copy(f"{ly.name}.cat{j}", u, real.slice(c0, u.C))
                    c0 += u.C
                x[j] = real
        assert all(isinstance(t, T) for t in x)
        return list(x)

    def _m_head(self, ly: _Layer):  # Detect, Segment, OBB, Pose, v10Detect: args [nc, ...] (+ the channel list parse_model appends, tasks.py:1075)
        m, name, args, arg = ly.m, ly.name, ly.args, ly.arg
        xs = ly.x if isinstance(ly.x, list) else [ly.x]
        assert all(isinstance(t, T) for t in xs)
        if m == "Segment":  # head.py:175-197, args [nc, nm, npr]; npr scaled like parse_model does (tasks.py:1082-1083)
            self.proto(name + ".proto", xs[0], self._scaled(args[2]), args[1])
            self.detect(name, xs, args[0], self.legacy, nm=args[1])
        elif m == "OBB":  # head.py:200-227, args [nc, ne]
            ne = 1 if isinstance(arg(1, 1), (list, tuple)) else arg(1, 1)
            if ne != 1:
                raise NotImplementedError(f"OBB with ne = {ne}: dist2rbox (utils/tal.py:404-423) decodes one angle")
            self.detect(name, xs, args[0], self.legacy, ne=ne)
        elif m == "Pose":
            # head.py:230-279, args [nc, kpt_shape].  Every pose yaml of the reference names the model's top-level kpt_shape
            # (tasks.py:981-985 evaluates the string; PoseModel.yaml holds the key, with a dataset's override applied, tasks.py:429-431),
            # and that form is the accelerated one: a head line that spells the pair out stays on the reference
            if arg(1, None) != "kpt_shape":
                raise NotImplementedError(f"{name}: Pose with the argument {arg(1, None)!r} (the yaml's form, the name 'kpt_shape', is accelerated)")
            ks = self.cfg.get("kpt_shape")
            if not isinstance(ks, (list, tuple)) or len(ks) != 2:
                raise NotImplementedError(f"{name}: the Pose head names kpt_shape, the model description has {ks!r} (a pair: keypoints, channels of each)")
            nkpt, ndim = int(ks[0]), int(ks[1])
            if ndim not in (2, 3) or not 1 <= nkpt <= 64:  # the limits of csrc/pose.hip and of the decode launch
                raise NotImplementedError(f"{name}: Pose with kpt_shape ({nkpt}, {ndim}): 1 to 64 keypoints of 2 or 3 channels are accelerated")
            self.detect(name, xs, args[0], self.legacy, nk=nkpt * ndim, kdim=ndim)
            self.meta.update(task="pose", nk=nkpt * ndim, kpt_shape=(nkpt, ndim))  # (only a pose plan's meta has these keys)
        elif m == "WorldDetect":
            # head.py:307-320, args [nc, embed, with_bn].  `nc` sizes c3 (head.py:313); the rows scored are the text features' (text_nc)
            if not ly.last:
                raise NotImplementedError(f"{name}: WorldDetect is accelerated as the last layer only")
            if not bool(arg(2, False)):
                raise NotImplementedError(f"{name}: WorldDetect with with_bn = False (ContrastiveHead, block.py:3591-3606: its per-pixel L2 "
                                          "normalisation of the embedding is not linear, so the head does not fold into a conv) is not accelerated")
            self.detect(name, xs, self.text_nc or args[0], True, world=(int(arg(1, 512)), args[0]))
            self.meta.update(world=True)
        elif m == "v10Detect":  # head.py:592-625: Detect with end2end = True and the light class branch whatever the graph holds
            if not ly.last:
                raise NotImplementedError(f"{name}: v10Detect is accelerated as the last layer only")
            self.detect(name, xs, args[0], False, end2end=True)
        else:
            self.detect(name, xs, args[0], self.legacy)

    def _m_classify(self, ly: _Layer):  # head.py:282-304, args [nc, k, s, p, g] (tasks.py:1016-1023 puts c1 in front)
        name, x, args, arg = ly.name, ly.x, ly.args, ly.arg
        if not isinstance(x, T):
            raise NotImplementedError(f"{name}: Classify fed by {len(x)} tensors (its torch.cat, head.py:298) is not accelerated")
        if not ly.last:
            raise NotImplementedError(f"{name}: Classify is accelerated as the last layer only")
        if (arg(1, 1), arg(2, 1), arg(3, None), arg(4, 1)) != (1, 1, None, 1):
            raise NotImplementedError(f"{name}: Classify with k, s, p, g = {args[1:5]} (the default 1x1 conv is accelerated)")
        # tasks.py:1019-1020: an output width that is not the class count is scaled like any other
        self.classify(name, x, args[0] if args[0] == self.cfg["nc"] else self._scaled(args[0]))

    # Module name -> (its lowering, whether args[0] is a channel count that parse_model width-scales: the lowering's ly.c2).  A new
    # module is one entry here and its lowering above; a module that is not here is not on the accelerated path
    LOWERINGS = {
        "Conv": (_m_conv, True), "DWConv": (_m_dwconv, True), "GhostConv": (_m_ghostconv, True), "GhostBottleneck": (_m_ghost_bottleneck, True),
        "C3": (_m_c3, True), "C3Ghost": (_m_c3, True), "C3k2": (_m_c3k2, True), "C3k2_gai": (_m_c3k2, True), "C2f": (_m_c2f, True),
        "C2fCIB": (_m_c2f, True), "C2fAttn": (_m_c2fattn, True), "C2": (_m_c2, True), "SCDown": (_m_scdown, True), "C2PSA": (_m_c2psa, True), "PSA": (_m_c2psa, True),
        "SPPF": (_m_spp, True), "SPP": (_m_spp, True), "SPPELAN": (_m_spp, True), "Bottleneck": (_m_bottleneck, True),
        "RepNCSPELAN4": (_m_elan, True), "ELAN1": (_m_elan, True), "AConv": (_m_down, True), "ADown": (_m_down, True),
        "MSCAAttention": (_m_attention, False), "ELA": (_m_attention, False), "nn.Upsample": (_m_upsample, False), "Concat": (_m_concat, False),
        "nn.ZeroPad2d": (_m_zeropad, False), "nn.MaxPool2d": (_m_maxpool, False), "nn.ConvTranspose2d": (_m_deconv, False),  # (scales c2 itself)
        "Detect": (_m_head, False), "Segment": (_m_head, False), "OBB": (_m_head, False), "Pose": (_m_head, False), "v10Detect": (_m_head, False),
        "WorldDetect": (_m_head, False),
        "Classify": (_m_classify, False),
        "nn.Identity": (_m_identity, False), "CBLinear": (_m_cblinear, False), "CBFuse": (_m_cbfuse, False),  # YOLOv9e (the widths are literal)
    }

    def _fuse_layer0(self, on: bool, kind: int, match):
        """Layer 0 (the image conv) and the one op of layer 1, fed by layer 0 alone, as one launch of `kind`: match(a, b) returns the fused
        op's own fields where the pair is that peephole's (else None).  Layer 0's map is then never materialised (layer_out[0] = None)."""
        if not on or len(self.ops) < 2 or self.ops[0]["kind"] != L.OP_CONV_FIRST:
            return
        a, b = self.ops[0], self.ops[1]
        mid = a["dst"]
        fields = match(a, b) if b.get("src0") is mid else None
        if fields is None:
            return
        # layer 0 must have no other reader.  A layer's map reaches an op through src0 / src1 / res alone: the list fields hold head maps,
        # scratch and, for CBFUSE, CBLinear outputs, which are no layer's map (only a CBFuse reads them) -- a kind that reads a layer's map
        # through box / cls would have to be looked at here as well
        for o in self.ops[2:]:
            for t in (o.get("src0"), o.get("src1"), o.get("res")):
                if t is not None and t.buf == mid.buf:
                    return
        self.buf_bytes[mid.buf] = 16  # never written
        self._emit(kind, a["name"] + "+" + b["name"].split(".")[-1], src0=a["src0"], dst=b["dst"], act=a["act"], wkey=a["wkey"],
                   in_dtype=self.in_dtype, **fields)
        self.ops[0:2] = [self.ops.pop()]  # (the two layers' flops are counted already)
        self.layer_out[self._first_layer] = None

    def _fuse_first_pool(self):
        """Peephole: layer 0 (image conv 3x3 s1 p1) + layer 1 (MaxPool2d(2, 2, 0)) -> one OP_FIRST_POOL launch (csrc/conv_first.hip)."""
        def match(a, b):
            if (b["kind"] == L.OP_MAXPOOL and (a["ksize"], a["stride"], a["pad"]) == (3, 1, 1) and b["level"] == 0
                    and kernel_takes("first_pool", a["dst"].C, self.H, self.W)):
                return dict(H=self.H, W=self.W, ksize=3, stride=1, pad=1, mfma_flops=a["mfma_flops"])
        self._fuse_layer0(self.fuse_first_pool, L.OP_FIRST_POOL, match)

    def _fuse_stem(self):
        """Peephole: layer 0 (image conv 3x3 s2) + layer 1 (3x3 s2 conv, the same activation) -> one OP_STEM launch (csrc/stem_fused.hip)."""
        def match(a, b):
            if (b["kind"] == L.OP_CONV and b.get("src1") is None and b.get("res") is None and b["ksize"] == 3 and b["stride"] == 2
                    and not b["out_f32"] and b["act"] and b["act"] == a["act"] and a["ksize"] == 3 and a["stride"] == 2
                    and kernel_takes("stem_fused", a["dst"].C, b["dst"].C, self.H, self.W)):
                return dict(ksize=3, stride=2, pad=1, wkey2=b["wkey"], mid_c=a["dst"].C, mfma_flops=a["mfma_flops"] + b["mfma_flops"])
        self._fuse_layer0(self.fuse_stem, L.OP_STEM, match)

    # ---- workspace layout -----------------------------------------------------------------------------------------
    def op_buffers(self, o: dict) -> List[int]:
        """Indices of the workspace buffers an op reads or writes (external slots excluded)."""
        views = [o.get(k) for k in VIEW_FIELDS] + [t for k in LIST_FIELDS for t in o.get(k) or []]
        return [t.buf for t in views if t is not None and t.buf < L.BSY_EXT_BASE]

    def max_view_elems(self) -> int:
        """Largest (pixels x row stride) of ONE image over the workspace views the ops name as source, destination or residual: the
        kernels keep element offsets in 32 bits, so the engine splits a batch when B times this (of the one-image plan) reaches 2^31.
        A C2f concat buffer is larger than the first conv's output."""
        views = [o.get(k) for o in self.ops for k in VIEW_FIELDS]
        return max([1] + [(t.H // 2) * (t.W // 2) * t.ld if t.up else t.H * t.W * t.ld for t in views if t is not None and t.buf < L.BSY_EXT_BASE])

    def buffer_lifetimes(self) -> List[Optional[Tuple[int, int]]]:
        """Per buffer: (first, last) index of the ops that touch it, or None for a buffer no op uses.  Ops on side lanes run
        concurrently with everything between their fork and the next join (csrc/engine.hip bsy_plan_run), so every buffer a
        lane op touches is kept alive over that whole region: the serial op order says nothing about when a lane runs."""
        n = len(self.ops)
        life: List[Optional[List[int]]] = [None] * len(self.buf_bytes)
        for i, o in enumerate(self.ops):
            for b in self.op_buffers(o):
                if life[b] is None:
                    life[b] = [i, i]
                else:
                    life[b][1] = i
        i = 0
        while i < n:
            if self.ops[i]["lane"] > 0:
                start = i
                end = n - 1  # the tail join of bsy_plan_run
                for j in range(i + 1, n):
                    if self.ops[j].get("join", 0):
                        end = j
                        break
                for j in range(start, end + 1):
                    if self.ops[j]["lane"] > 0:
                        for b in self.op_buffers(self.ops[j]):
                            life[b][0] = min(life[b][0], start)
                            life[b][1] = max(life[b][1], end)
                i = end + 1
            else:
                i += 1
        return [tuple(x) if x is not None else None for x in life]

    def assign_offsets(self, reuse: bool = True) -> Tuple[List[int], int]:
        """Byte offset of every buffer inside one arena and the arena size.  reuse: buffers whose lifetimes are disjoint may
        share addresses (greedy by size: each buffer, largest first, takes the lowest offset free of every already placed
        buffer it is live together with) -- YOLO11s at batch 64, 640 x 640: 3.8 GB of buffers in a 1.3 GB arena."""
        sizes = [(b + 255) & ~255 for b in self.buf_bytes]
        offs = [0] * len(sizes)
        if not reuse:
            off = 0
            for i, sz in enumerate(sizes):
                offs[i] = off
                off += sz
            return offs, off
        life = self.buffer_lifetimes()
        placed: List[int] = []
        top = 0
        for i in sorted(range(len(sizes)), key=lambda k: (-sizes[k], k)):
            if life[i] is None or sizes[i] == 0:
                continue
            busy = sorted((offs[j], offs[j] + sizes[j]) for j in placed
                          if not (life[j][1] < life[i][0] or life[i][1] < life[j][0]))
            at = 0
            for lo, hi in busy:
                if at + sizes[i] <= lo:
                    break
                at = max(at, hi)
            offs[i] = at
            placed.append(i)
            top = max(top, at + sizes[i])
        return offs, top

    def conv_signature(self, o: dict) -> Optional[tuple]:
        """What decides which kernel configuration is fastest for a conv op (and which are valid): the key of the engine's
        autotune cache.  None for ops the autotuner does not touch."""
        if o["kind"] != L.OP_CONV or self.f32_mode:
            return None
        s0, s1, d, r = o["src0"], o.get("src1"), o["dst"], o.get("res")
        return (self.B, o["H"], o["W"], s0.C, s0.ld, int(s0.up), s1.C if s1 else 0, s1.ld if s1 else 0, int(s1.up) if s1 else 0,
                o.get("cout", d.C), d.ld, o["ksize"], o["stride"], int(r is not None), r.ld if r is not None else 0,
                o.get("out_f32", 0), o.get("dst_scale", 1), o.get("act", 0), o.get("ksplit", 0))

    # ---- serialisation ------------------------------------------------------------------------------------------
    def c_ops(self):
        def v(t):
            return L.View(*(t.view() if t is not None else L.NO_VIEW))

        def offsets(key):
            w = self.wrecs[key]
            assert w.w_off >= 0, "pack weights before serialising"
            return w.w_off, w.b_off

        arr = (L.Op * len(self.ops))()
        for o, d in zip(arr, self.ops):
            if d["kind"] == L.OP_ELA:  # the three sigmoids are known once the weights are packed (WRec.coef).  They stay in the plan's
                # own op: a side effect of serialising that nothing reads today (the device gets them through `o` below)
                cf = self.wrecs[d["wkey"]].coef
                d["scale"], d["lvl_stride"] = cf[0], [cf[1], cf[2]]
            o.kind, o.lane, o.tuned_cfg = d["kind"], d["lane"], 0
            o.B, o.H, o.W, o.OH, o.OW = self.B, d["H"], d["W"], d["OH"], d["OW"]
            o.prec = (2 if self.split_f16 else 1) if self.f32_mode else 0
            for f, default in SCALAR_FIELDS:  # (level: the mode of MAXPOOL / POOL_DOWN as well)
                setattr(o, f, d.get(f, default))
            for f in VIEW_FIELDS:
                setattr(o, f, v(d.get(f)))
            o.up0 = int(bool(d.get("src0") and d["src0"].up))
            o.up1 = int(bool(d.get("src1") and d["src1"].up))
            for f in LIST_FIELDS:
                views, member = d.get(f, ()), getattr(o, f)
                for j in range(L.BSY_MAX_LEVELS):
                    member[j] = v(views[j] if j < len(views) else None)
            for f, default in LEVEL_FIELDS:
                values, member = d.get(f, ()), getattr(o, f)
                for j in range(L.BSY_MAX_LEVELS):
                    member[j] = values[j] if j < len(values) else default
            if "wkey" in d:
                o.w_off, o.b_off = offsets(d["wkey"])
            if "wkey2" in d:
                o.w2_off, o.b2_off = offsets(d["wkey2"])
            for j, k in enumerate(d.get("wkeys", [])):
                o.aux_off[2 * j], o.aux_off[2 * j + 1] = offsets(k)
        return arr
