"""Engine wrapper: owns a bsy_engine (weights in HBM, ONE activation arena) and an LRU set of bsy_plans, one per input shape.

`YoloEngine.__call__(im)` has the calling convention AutoBackend expects from an in-memory model
(nn/autobackend.py:524: ``self.model(im, augment=, visualize=, embed=)`` -> ``(y, x_list)``, head.py:74), with
``im`` a contiguous BCHW fp16/fp32 tensor on the engine's device.  PyTorch is only used for device memory and
the current stream; all compute goes through libbsyolo_hip.so.

An engine built from a classification graph (a `Classify` head) returns what Classify.forward returns in eval (head.py:304): ``(y, x)``,
the softmax and the logits, (B, nc) each in the input's dtype.  The top-min(nc, 5) classes of the same launch -- what the reference's
predictor and validator take with an argsort -- are kept as ``engine.last_topk = (idx int32, val f32)``, (B, k) device rows of the
LAST forward (in graph mode they belong to the ring slot of that forward, like y).

An engine built from a pose graph (a `Pose` head) returns what Pose.forward returns in eval (head.py:250): ``(y, (x_list, kpt))`` with
y (B, 4 + nc + nk, A) -- the decoded keypoint rows behind the scores -- and kpt (B, nk, A) the raw keypoint logits;
``want_raw=False`` gives ``(y, ([None] * nl, None))``.

An engine built from a YOLOv10 graph (a `v10Detect` head) returns what v10Detect.forward_end2end returns in eval (head.py:96-98):
``(rows, {"one2many": [...], "one2one": [...]})`` with rows (B, min(max_det, A), 6) fp32 -- [x1, y1, x2, y2, score, class], the top-k of
the one2one head (BSY_OP_E2E_TOPK) -- and the raw maps of both head copies, BCHW in the input's dtype.  ``want_raw=False`` gives
``(rows, {"one2many": [None] * nl, "one2one": [None] * nl})`` from a plan of its own that never runs the one2many branches.  The
pre-top-k tensor (B, 4 + nc, A) of the last ``want_raw=True`` forward is kept as ``engine.last_e2e_pre`` (as last_topk is).

An engine built from a YOLO-World v2 graph (C2fAttn blocks, a `WorldDetect` head) returns what WorldDetect.forward returns in eval: ``(y,
x_list)`` with y (B, 4 + nc, A) and raw maps of 64 + nc channels, nc the ROWS of the text features it was built with (``txt_feats=``, the
model's ``txt_feats``, or the state dict's reserved key "txt_feats"); the text is constant per engine and folded into its weights.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from collections import OrderedDict
from typing import Dict, List, Mapping, Optional, Tuple

import torch

from . import lib as L
from . import ops as O
from . import tta as T
from .plan import SWITCHES, Plan
from .weights import BN_EPS, TXT_KEY, adopt_offsets, pack_plan_weights, repconv_form

_DTYPES = {"int32": torch.int32, "float32": torch.float32}  # Plan.outputs' dtypes besides "io", the forward's own


def _outputs(plan: Plan, want_raw: bool, device, dtype) -> Dict[str, Optional[torch.Tensor]]:
    """Fresh tensors for the plan's external outputs (Plan.outputs), by name; None for the ones only a want_raw caller has."""
    return {o.name: torch.empty(o.shape, dtype=_DTYPES.get(o.dtype, dtype), device=device) if want_raw or not o.raw_only else None
            for o in plan.outputs.values()}


def _bind(plan: Plan, im: torch.Tensor, outs: Mapping[str, Optional[torch.Tensor]]):
    """(void* array, length) of the plan's external slots: the image and every output `outs` holds; the others stay unbound (NULL), and
    the launches skip their stores (include/bsyolo.h, bsy_plan_run)."""
    ptrs = [None] * (1 + max(o.slot for o in plan.outputs.values()))
    ptrs[Plan.EXT_IMG] = im.data_ptr()
    for o in plan.outputs.values():
        if outs.get(o.name) is not None:
            ptrs[o.slot] = outs[o.name].data_ptr()
    return (C.c_void_p * len(ptrs))(*ptrs), len(ptrs)


def pack_outputs(meta: Mapping, outs: Mapping[str, Optional[torch.Tensor]]):
    """What the model's forward returns in eval, from the outputs by name (y already carries the rows behind the scores)."""
    if meta.get("end2end"):  # v10Detect.forward_end2end (head.py:98): (rows, {"one2many": x, "one2one": one2one})
        nl = range(len(meta["levels"]))
        return outs["rows"], {"one2many": [outs.get(f"o2m{l}") for l in nl], "one2one": [outs[f"o2o{l}"] for l in nl]}
    y = outs["y"]
    if meta.get("task") == "classify":  # Classify.forward (head.py:304): (softmax, logits)
        return y, outs["x"]
    raws = [outs[f"raw{l}"] for l in range(len(meta["levels"]))]
    if meta["nm"]:  # Segment.forward (head.py:197): (cat(y, mc), (raw, mc, proto))
        return y, (raws, y[:, 4 + meta["nc"]:], outs["proto"])
    if meta["ne"]:  # OBB.forward (head.py:223): (cat(y, angle), (raw, angle))
        return y, (raws, y[:, 4 + meta["nc"]:])
    if meta.get("nk", 0):  # Pose.forward (head.py:250): (cat(y, pred_kpt), (raw, kpt))
        return y, (raws, outs["kpt"])
    return y, raws  # Detect.forward (head.py:74)


def cat_outputs(chunks: List[Mapping[str, Optional[torch.Tensor]]]) -> Dict[str, Optional[torch.Tensor]]:
    """The outputs of consecutive slices of a batch, joined along dim 0 (an output no chunk has stays None)."""
    return {k: None if v is None else torch.cat([c[k] for c in chunks]) for k, v in chunks[0].items()}


def sppf_form(model, cfg: dict) -> str:
    """Plan's `sppf_act` of a live reference model.  Read under a ReLU graph (`activation: nn.ReLU()`) alone -- every other graph
    answers "silu", which the plan ignores there.  Under ReLU every SPPF layer of the yaml is looked at: "relu" where cv1 and cv2 hold
    nn.ReLU, "silu" where both hold nn.SiLU; layers that cannot be reached, another activation class, or convs that disagree (with each
    other or between two SPPF layers) raise NotImplementedError: one plan parameter cannot describe that model."""
    if cfg.get("activation") != "nn.ReLU()":
        return "silu"
    forms = set()
    for i, layer in enumerate(list(cfg.get("backbone", [])) + list(cfg.get("head", []))):
        if layer[2] != "SPPF":
            continue
        try:
            acts = [model.model[i].cv1.act, model.model[i].cv2.act]
        except (AttributeError, IndexError, TypeError, KeyError) as e:
            raise NotImplementedError(f"model.{i}: cannot read SPPF's activations off the model ({type(e).__name__}: {e}); pass sppf_act") from e
        for name, act in zip(("cv1", "cv2"), acts):
            if not isinstance(act, (torch.nn.ReLU, torch.nn.SiLU)):
                raise NotImplementedError(f"model.{i}.{name}: SPPF's activation is {act}: nn.SiLU and nn.ReLU are accelerated")
            forms.add("relu" if isinstance(act, torch.nn.ReLU) else "silu")
    if len(forms) > 1:
        raise NotImplementedError("the model's SPPF convs disagree on their activation (nn.SiLU in some, nn.ReLU in others): not accelerated")
    return forms.pop() if forms else "silu"


class YoloEngine:
    def __init__(self, cfg: dict, state_dict: Mapping[str, torch.Tensor], device: int = 0, bn_eps: float = BN_EPS,
                 autotune: Optional[bool] = None, max_plans: Optional[int] = None, precision: str = "fp16", graph: Optional[bool] = None,
                 graph_ring: int = 3, latency: Optional[bool] = None, repconv: Optional[str] = None, max_det: int = 300,
                 sppf_act: Optional[str] = None, txt_feats: Optional[torch.Tensor] = None, **switches: Optional[bool]):
        """switches: the fusion switches of plan.SWITCHES (fuse_stem=False, ...), handed to every plan; None or absent = the switch's
        environment variable, on where that is unset.  max_det: the rows a v10Detect head's top-k keeps (1 .. 4096; other heads ignore it).
        state_dict: a mapping, or the reference model itself (its state_dict() is taken).  sppf_act: Plan's parameter of that name, what
        SPPF's two convs apply in a graph under `activation: nn.ReLU()` (YOLOv6) -- "silu" in a model this fork built from the yaml, "relu"
        in an upstream-pickled one.  None reads it off the model (sppf_form below) where `state_dict` is one; a bare state dict does not
        say which form it came from, so None then means "silu": pass "relu" for an upstream checkpoint's state dict.
        txt_feats: a YOLO-World graph's text features, (nc, E) or (1, nc, E): this tensor, else the model's `txt_feats` attribute where
        `state_dict` is a model, else the state dict's key "txt_feats".  Their row count is the number of classes the engine scores
        (Plan's text_nc, `engine.nc`); cfg["nc"] keeps sizing the head's hidden width.  Other graphs ignore the argument."""
        world = (list(cfg.get("head", [])) or [[0, 0, ""]])[-1][2] == "WorldDetect"
        if isinstance(state_dict, torch.nn.Module):
            sppf_act = sppf_act or sppf_form(state_dict, cfg)
            if txt_feats is None and world:
                txt_feats = getattr(state_dict, "txt_feats", None)
            state_dict = {k: v.detach().float().cpu() for k, v in state_dict.state_dict().items()}
        self.text_nc, self.txt_feats = None, None  # (txt_feats: the text the weights in use were folded with, kept for load_weights)
        if world:
            state_dict = self._with_text(state_dict, txt_feats)
            self.text_nc = int(state_dict[TXT_KEY].shape[-2])
        self.sppf_act = sppf_act or "silu"
        if not set(switches) <= set(SWITCHES):
            raise TypeError(f"YoloEngine() got an unexpected keyword argument {sorted(set(switches) - set(SWITCHES))[0]!r}")
        if not torch.cuda.is_available():
            raise RuntimeError("bs_yolo_amd needs a ROCm GPU (there is no CPU fallback)")
        self.cfg = cfg
        # "fp32": the correctness mode -- fp32 activation storage and arithmetic (csrc/ref32.hip, conv32_mfma.hip), for callers that
        # expect the fp32 model's numbers bit-reproducibly (|dscore| <= 1e-5 against the fp32 reference).  "fp32x": the same storage
        # and non-conv kernels, dense convs on the fp16 matrix pipe with split-f16 operands (csrc/conv32x_mfma.hip): the
        # north-star's 1e-3 at several times the fp32 mode's throughput.  "fp16" is the product path.
        self.precision = precision
        # latency mode (BSY_LATENCY=1): split-K on the long-K, few-tile conv layers -- for small per-rank batches (a rank's 8- or
        # 16-image share of a strong-scaled batch).  The split factors depend on the layer shape only, so any batch split returns the
        # bits of the whole batch IN THIS MODE; they differ from the default mode's by f32 summation order (Plan.split_factors).
        self.latency = (os.environ.get("BSY_LATENCY", "0") == "1") if latency is None else bool(latency)
        self.device = torch.device("cuda", device)
        self._h = C.c_void_p()
        L.check(L.lib.bsy_engine_create(device, C.byref(self._h)))
        # plans: least-recently-used first.  val runs with rect=True (engine/model.py:635; per-batch shapes,
        # data/base.py:261-284) and predict's `auto` letterbox also varies (H, W): a plan is cheap to rebuild (host-side
        # flattening + a handful of streams / events), its activations live in the engine's shared arena and its tuning in
        # `_tune_cache`, so old shapes are simply dropped
        self._plans: "OrderedDict[Tuple, Tuple]" = OrderedDict()
        self.max_plans = int(os.environ.get("BSY_MAX_PLANS", "8")) if max_plans is None else int(max_plans)
        self._tuned = set()
        self._elems: Dict[Tuple[int, int], int] = {}
        # autotune results keyed by conv shape (Plan.conv_signature), shared by every plan of this engine and, with
        # BSY_TUNE_CACHE=<file>, across processes.  `tune_stats` counts what bsy_plan_autotune had to time.
        self._tune_cache: Dict[tuple, int] = {}
        # second level: the same layer (channels, kernel, stride, epilogue) at a similar size (pixel count within a factor of
        # two) reuses the winner without timing -- rect batches differ from each other by a few rows or columns
        self._tune_family: Dict[tuple, int] = {}
        self.tune_stats = {"timed_ops": 0, "cached_ops": 0, "family_ops": 0, "autotune_calls": 0}
        # how conv configurations are timed (see _autotune): "1" every candidate in place (default), anything else one layer
        # at a time (bsy_plan_autotune)
        self.tune_mode = os.environ.get("BSY_TUNE_IN_PLACE", "1")
        self._tune_file = os.environ.get("BSY_TUNE_CACHE")
        if self._tune_file and os.path.exists(self._tune_file):
            try:
                self._tune_cache = {tuple(k): int(v) for k, v in json.load(open(self._tune_file))}
                for k, v in self._tune_cache.items():
                    self._tune_family.setdefault(self._family(k), v)
            except (OSError, ValueError):
                self._tune_cache = {}
        # liveness-based buffer reuse (Plan.assign_offsets).  Off under BSY_ARENA_REUSE=0 (tests that read intermediate
        # layers back) and under BSY_PLAN_GUARD (guard bands behind every buffer: the plan then owns a private workspace)
        self.reuse = os.environ.get("BSY_ARENA_REUSE", "1") != "0" and not os.environ.get("BSY_PLAN_GUARD")
        # Graph mode (opt-in: graph=True / BSY_GRAPH=1): the forward of a shape is captured once per set of buffer addresses and
        # replayed as ONE hipGraph launch (bsy_plan_graph_launch) -- what a rank needs at its 8- or 16-image share of a strong-
        # scaled batch, where 70-odd launches of 4-15 us are bound by the host's launch rate.  The graph bakes addresses in, so the
        # outputs come from a ring of `graph_ring` preallocated sets per shape: a returned `y` is overwritten by the graph_ring-th
        # forward after it (the reference's predict / val loops consume `preds` within the iteration, engine/predictor.py:254-262).
        # Head lanes are on at every size in this mode (fork / join are graph edges).
        self.graph = (os.environ.get("BSY_GRAPH", "0") == "1") if graph is None else bool(graph)
        self.graph_ring = max(1, int(graph_ring))
        self._rings: Dict[Tuple, dict] = {}
        self._gstream = None
        # All plans of an engine share ONE activation arena (liveness-packed): two forwards must never be in flight at once.  The
        # reference serialises predict() with a lock (engine/predictor.py:113,229); here a host lock covers the enqueue and an event
        # recorded behind every forward makes a forward enqueued on ANOTHER stream wait for the previous one (same stream: ordered
        # anyway, no event wait is issued).
        import threading
        self._lock = threading.RLock()
        self._last_done = None
        self._last_stream = None
        self.graph_stats = {"captures": 0, "replays": 0, "eager": 0}
        self._tta_geom: Dict[Tuple[int, int], list] = {}  # (H, W) -> tta.Pass list (forward_augment)
        self._tta_bufs: "OrderedDict[Tuple, torch.Tensor]" = OrderedDict()  # scaled TTA inputs per (pass, B, PH, PW, dtype), LRU
        self.autotune = ((os.environ.get("BSY_AUTOTUNE", "1") != "0") if autotune is None else bool(autotune)) and precision == "fp16"
        self.switches = dict(switches)
        # YOLOv9 graphs: which RepConv the RepBottlenecks hold (Plan's `repconv`); None reads it off the state dict's keys
        self.repconv = repconv or repconv_form(state_dict)
        self.max_det = int(max_det)
        # pack once with a throw-away plan (op list structure does not depend on the input size).  one2many: a v10Detect head's plan with
        # both head copies, so that the blob holds every weight and the rows-only plans adopt their share of its offsets
        self._packed = Plan(cfg, 1, 64, 64, one2many=True, **self._fuse_kw())
        blob = pack_plan_weights(self._packed, state_dict, bn_eps)
        self.weight_bytes = len(blob)
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        L.check(L.lib.bsy_engine_load_weights(self._h, buf, len(blob)))
        self.txt_feats = state_dict[TXT_KEY] if world else None
        self.meta = dict(self._packed.meta)
        self.nc = self.meta["nc"]
        self.stride = torch.tensor(self.meta["strides"])
        self.nl = len(self.meta["levels"])  # detection levels: 3, or 4 on the P2 / P6 graphs
        self.max_stride = int(max(self.meta["strides"]))  # inputs are multiples of it: 32, 64 on a P6 graph
        self.names = {i: f"{i}" for i in range(self.nc)}
        self.task = self.meta.get("task", "detect")  # "classify": forward returns (y, x), see the module docstring
        self.last_topk: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self.end2end = bool(self.meta.get("end2end"))  # a v10Detect head: forward returns (rows, {...}), see the module docstring
        self.last_e2e_pre: Optional[torch.Tensor] = None

    @staticmethod
    def _with_text(state_dict: Mapping[str, torch.Tensor], txt_feats) -> Mapping[str, torch.Tensor]:
        """`state_dict` with the text features under the reserved key (weights.TXT_KEY): `txt_feats` where given, else what it holds."""
        if txt_feats is not None:
            state_dict = dict(state_dict)
            state_dict[TXT_KEY] = torch.as_tensor(txt_feats).detach().float().cpu()
        if TXT_KEY not in state_dict:
            raise ValueError("a YOLO-World graph needs its text features: txt_feats=, the model's txt_feats, or state_dict['txt_feats']")
        t = state_dict[TXT_KEY]
        if t.dim() == 3 and t.shape[0] != 1:
            raise NotImplementedError(f"txt_feats of shape {tuple(t.shape)}: per-image text features are not accelerated (one set per call)")
        if t.dim() not in (2, 3):
            raise ValueError(f"txt_feats of shape {tuple(t.shape)}: (nc, E) or (1, nc, E)")
        return state_dict

    def load_weights(self, state_dict: Mapping[str, torch.Tensor], bn_eps: float = BN_EPS, txt_feats: Optional[torch.Tensor] = None) -> None:
        """Replace the engine's weights in place (same graph, new values: an EMA update, a fine-tuned checkpoint).  Plans, tuning and
        the arena are kept; the library synchronises the device before it frees the old blob and drops every captured graph (they
        hold addresses inside it: include/bsyolo.h, bsy_engine_load_weights).  txt_feats (a YOLO-World engine): new text features of the
        SAME row count -- the guide and class records are folded again; another row count is another plan and raises ValueError.  Without
        it, and without the reserved key in `state_dict` (a model's state_dict() never holds it), the text in use is folded into the new weights."""
        if self.text_nc is not None:
            if txt_feats is None and TXT_KEY not in state_dict:
                txt_feats = self.txt_feats
            state_dict = self._with_text(state_dict, txt_feats)
        with self._lock:
            blob = pack_plan_weights(self._packed, state_dict, bn_eps)
            if len(blob) != self.weight_bytes:
                raise ValueError(f"state_dict packs to {len(blob)} bytes, the engine was built for {self.weight_bytes}")
            for plan, _ in self._plans.values():
                adopt_offsets(plan, self._packed)
            buf = (C.c_char * len(blob)).from_buffer_copy(blob)
            L.check(L.lib.bsy_engine_load_weights(self._h, buf, len(blob)))
            if self.text_nc is not None:
                self.txt_feats = state_dict[TXT_KEY]

    def _fuse_kw(self):
        return dict(self.switches, precision=self.precision, lanes=True if self.graph else None, latency=self.latency, repconv=self.repconv,
                    max_det=self.max_det, sppf_act=self.sppf_act, **({} if self.text_nc is None else {"text_nc": self.text_nc}))

    # -- plans --------------------------------------------------------------------------------------------------
    def plan_for(self, B: int, H: int, W: int, in_dtype: torch.dtype, out_dtype: torch.dtype, one2many: bool = False):
        """one2many: an end2end engine's plan with the one2many branches, built when a want_raw caller first needs it (others: ignored)."""
        one2many = bool(one2many) and self.end2end
        key = (B, H, W, in_dtype, out_dtype) + ((True,) if one2many else ())
        hit = self._plans.get(key)
        if hit is not None:
            self._plans.move_to_end(key)
            return hit
        gs = self.max_stride
        if H % gs or W % gs:
            raise ValueError(f"input {H}x{W} must be a multiple of the max stride {gs} (utils/checks.py:120-172)")
        plan = Plan(self.cfg, B, H, W, L.dtype_code(in_dtype), L.dtype_code(out_dtype), one2many=one2many, **self._fuse_kw())
        adopt_offsets(plan, self._packed)
        ops = plan.c_ops()
        sizes = (C.c_int64 * len(plan.buf_bytes))(*plan.buf_bytes)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            if os.environ.get("BSY_PLAN_GUARD"):  # test aid: private workspace with guard bands, no aliasing
                L.check(L.lib.bsy_plan_create(self._h, ops, len(plan.ops), sizes, len(plan.buf_bytes), C.byref(h)))
                plan.arena_bytes = sum((b + 255) & ~255 for b in plan.buf_bytes)
            else:
                offs, arena = plan.assign_offsets(self.reuse)
                plan.arena_bytes = arena
                L.check(L.lib.bsy_plan_create_arena(self._h, ops, len(plan.ops), sizes, (C.c_int64 * len(offs))(*offs),
                                                    len(offs), arena, C.byref(h)))
        # conv shapes an earlier plan (or an earlier process, BSY_TUNE_CACHE) already tuned: preset, not re-timed
        plan.conv_sigs = [plan.conv_signature(o) for o in plan.ops]
        for sg in plan.conv_sigs:
            if sg is not None and sg not in self._tune_cache and self._family(sg) in self._tune_family:
                self._tune_cache[sg] = self._tune_family[self._family(sg)]
                self.tune_stats["family_ops"] += 1
        preset = (C.c_int32 * len(plan.ops))(*[self._tune_cache.get(sg, -1) if sg is not None else -1 for sg in plan.conv_sigs])
        L.check(L.lib.bsy_plan_set_tuning(h, preset, len(plan.ops)))
        while len(self._plans) >= max(self.max_plans, 1):  # evict the least recently used shape
            old_key, (_, old) = self._plans.popitem(last=False)
            L.lib.bsy_plan_destroy(old)
            for rk in [k for k in self._rings if k[0] == old_key]:
                del self._rings[rk]
        plan.key = key
        self._plans[key] = (plan, h)
        return plan, h

    @property
    def arena_bytes(self) -> int:
        """Bytes of the activation arena all plans of this engine share (the largest plan so far)."""
        return int(L.lib.bsy_engine_arena_bytes(self._h))

    @staticmethod
    def _family(sg: tuple) -> tuple:
        B, H, W = sg[:3]
        return sg[3:] + (int(round(math.log2(max(B * H * W, 1)))),)

    def _autotune(self, plan, h, ext, n, stream):
        """First forward of a shape: time the candidate configurations of the conv ops whose shape has not been tuned yet
        (bsy_plan_autotune skips preset ops) and remember the winners by conv shape."""
        # presets that came from the tune file or from a similar-sized shape's entry may not fit this shape (another library version,
        # another alignment): drop them from the caches and from the plan, so that they are timed below instead of being persisted
        nops = len(plan.ops)
        valid = (C.c_int32 * nops)()
        L.check(L.lib.bsy_plan_check_tuning(h, ext, n, valid, nops))
        bad = [i for i in range(nops) if valid[i] == 0]
        if bad:
            clear = (C.c_int32 * nops)(*([-1] * nops))
            for i in bad:
                sg = plan.conv_sigs[i]
                cfg = self._tune_cache.pop(sg, None)
                if cfg is not None and self._tune_family.get(self._family(sg)) == cfg:
                    del self._tune_family[self._family(sg)]
                clear[i] = -2
            L.check(L.lib.bsy_plan_set_tuning(h, clear, nops))
            self.tune_stats["invalid_presets"] = self.tune_stats.get("invalid_presets", 0) + len(bad)
        todo = sum(1 for sg in plan.conv_sigs if sg is not None and sg not in self._tune_cache)
        self.tune_stats["autotune_calls"] += 1
        self.tune_stats["timed_ops"] += todo
        self.tune_stats["cached_ops"] += sum(1 for sg in plan.conv_sigs if sg is not None) - todo
        if self.tune_mode == "1":
            # every candidate of every new conv shape timed where it runs: pass k of the forward runs candidate k of all of them
            L.check(L.lib.bsy_plan_autotune_in_place(h, ext, n, C.c_void_p(stream), 3))
        else:
            L.check(L.lib.bsy_plan_autotune(h, ext, n, C.c_void_p(stream)))
        if todo:
            out = (C.c_int32 * nops)()
            L.check(L.lib.bsy_plan_get_tuning(h, out, nops))
            for sg, c in zip(plan.conv_sigs, out):
                if sg is not None and c >= 0:
                    self._tune_cache.setdefault(sg, int(c))
                    self._tune_family.setdefault(self._family(sg), int(c))
            if self._tune_file:
                try:
                    tmp = self._tune_file + f".{os.getpid()}.tmp"
                    json.dump([[list(k), v] for k, v in self._tune_cache.items()], open(tmp, "w"))
                    os.replace(tmp, self._tune_file)
                except OSError:
                    pass

    def _max_view_elems(self, H: int, W: int) -> int:
        """Plan.max_view_elems of ONE image at this size: a batch is split when B times this reaches 2^31 (forward)."""
        hit = self._elems.get((H, W))
        if hit is None:
            hit = self._elems[(H, W)] = Plan(self.cfg, 1, H, W, **self._fuse_kw()).max_view_elems()
        return hit

    @staticmethod
    def _dense(im: torch.Tensor) -> torch.Tensor:
        """`im` contiguous AND with its first element on a 16-byte boundary.  contiguous() keeps a contiguous view at an odd storage
        offset as it is, and the fused stem (csrc/stem_fused.hip: 4-pixel vector loads) refuses such a pointer where the unfused plan
        takes the element-wise load; such a view is copied, so every plan sees the same aligned image (one elementwise launch on the
        current stream; in graph mode a copy at a new address is captured like any other new input)."""
        im = im.contiguous()
        return im.clone() if im.data_ptr() % 16 else im

    def forward(self, im: torch.Tensor, want_raw: bool = True):
        if im.device != self.device:
            raise ValueError(f"input on {im.device}, engine on {self.device}")
        if im.dtype not in (torch.float16, torch.float32):
            raise TypeError("input must be fp16 or fp32 (BCHW, 0..1)")
        im = self._dense(im)
        B, Cc, H, W = im.shape
        if Cc != 3:
            raise ValueError("expected 3 input channels")
        if H % self.max_stride or W % self.max_stride:  # (before any plan of this size is built: the graph walk asserts on such maps)
            raise ValueError(f"input {H}x{W} must be a multiple of the max stride {self.max_stride} (utils/checks.py:120-172)")
        outs = self._forward_outs(im, want_raw)
        if "topk_idx" in outs:  # a classify plan's rows (of the whole batch where it was split)
            self.last_topk = (outs["topk_idx"], outs["topk_val"])
        if self.end2end and want_raw:  # what the rows were selected from (of the whole batch where it was split)
            self.last_e2e_pre = outs["pre"]
        return pack_outputs(self.meta, outs)

    def _forward_outs(self, im, want_raw):
        """The outputs of one forward by name (Plan.outputs)."""
        B, _, H, W = im.shape
        # the kernels keep element offsets in 32 bits: split batches whose largest activation would exceed 2^31
        # elements (e.g. 256 x 1280x1280) into equal chunks -- images are independent
        big = self._max_view_elems(H, W)
        if B > 1 and B * big >= (1 << 31) - (1 << 24):
            n_chunks = -(-B * big // ((1 << 31) - (1 << 24)))
            step = -(-B // n_chunks)
            return cat_outputs([self._forward_outs(self._dense(im[i:i + step]), want_raw) for i in range(0, B, step)])
        with self._lock:  # plan table, arena and launch order are shared state
            plan, h = self.plan_for(B, H, W, im.dtype, im.dtype, one2many=want_raw)
            outs = self._output_set(plan, im, want_raw)
            self._run(plan, h, *_bind(plan, im, outs), im, B, H, W)
            return outs

    def _output_set(self, plan, im, want_raw):
        """The output tensors of one forward: fresh ones (_outputs), or in graph mode the next set of this shape's ring -- the captured
        graphs hold their addresses."""
        if not self.graph:
            return _outputs(plan, want_raw, self.device, im.dtype)
        B, _, H, W = im.shape
        ring = self._rings.setdefault((plan.key, bool(want_raw)), {"i": 0, "slots": []})
        if len(ring["slots"]) < self.graph_ring:
            ring["slots"].append(_outputs(plan, want_raw, self.device, im.dtype))
        ring["i"] += 1
        return ring["slots"][(ring["i"] - 1) % len(ring["slots"])]

    def _run(self, plan, h, ext, n, im, B, H, W):
        """One forward of `plan` on the current stream with the external slots `ext`: ordered behind the previous forward, autotuned
        on the first call of a shape, replayed as a graph in graph mode."""
        cur_stream = torch.cuda.current_stream(self.device)
        stream = cur_stream.cuda_stream
        if self._last_done is not None and self._last_stream != stream:
            cur_stream.wait_event(self._last_done)  # the arena is still owned by a forward on another stream
        if self.autotune and plan.key not in self._tuned:
            # first call for this shape: pick the fastest kernel configuration per conv op (runs the plan once)
            self._tuned.add(plan.key)
            self._autotune(plan, h, ext, n, stream)
        if self.graph:
            how = C.c_int(-1)
            if stream == 0:
                # the legacy default stream cannot be captured: capture / replay on a stream of the engine's, ordered after the
                # caller's work and joined back into it (two event pairs per forward)
                cur = torch.cuda.current_stream(self.device)
                if self._gstream is None:
                    self._gstream = torch.cuda.Stream(device=self.device)
                self._gstream.wait_stream(cur)
                im.record_stream(self._gstream)
                L.check(L.lib.bsy_plan_graph_launch(h, ext, n, C.c_void_p(self._gstream.cuda_stream), C.byref(how)))
                cur.wait_stream(self._gstream)
            else:
                L.check(L.lib.bsy_plan_graph_launch(h, ext, n, C.c_void_p(stream), C.byref(how)))
            self.graph_stats[{1: "captures", 0: "replays"}.get(how.value, "eager")] += 1
            if how.value == 1 and self.graph_stats["captures"] > 4 * self.graph_ring + 4 and not getattr(self, "_graph_warned", False):
                # the graph key holds the INPUT pointer: callers that hand over a freshly allocated image tensor per call re-capture
                # (and re-instantiate) on almost every forward -- slower than the eager replay; say so once
                self._graph_warned = True
                import logging
                logging.getLogger("bs_yolo_amd").warning(
                    "graph mode has captured %d graphs (%d replays): inputs arrive at new addresses on every call, so every forward is "
                    "re-captured.  Reuse the input tensor (copy_ into one buffer per shape) or switch graph mode off.",
                    self.graph_stats["captures"], self.graph_stats["replays"])
        else:
            L.check(L.lib.bsy_plan_run(h, ext, n, C.c_void_p(stream)))
        if self._last_done is None:
            self._last_done = torch.cuda.Event()
        self._last_done.record(cur_stream)
        self._last_stream = stream

    def tuning(self, B, H, W, dtype=torch.float16):
        plan, h = self.plan_for(B, H, W, dtype, dtype)
        out = (C.c_int32 * len(plan.ops))()
        L.check(L.lib.bsy_plan_get_tuning(h, out, len(plan.ops)))
        return [(o["name"], int(c)) for o, c in zip(plan.ops, out) if c >= 0]

    def __call__(self, im, augment=False, visualize=False, embed=None, want_raw=True):
        if augment:  # tasks.py:134-136: augment wins over visualize / embed
            return self.forward_augment(im)
        if visualize or embed:
            raise NotImplementedError("visualize/embed fall back to the reference graph (tasks.py:137-164)")
        return self.forward(im, want_raw)

    def tta_geometry(self, H: int, W: int):
        """The TTA passes of an (H, W) input (bs_yolo_amd/tta.py), their windows from the plans' detection levels."""
        hit = self._tta_geom.get((H, W))
        if hit is None:
            levels = lambda h, w: Plan(self.cfg, 1, h, w, **self._fuse_kw()).meta["levels"]  # noqa: E731
            hit = self._tta_geom[(H, W)] = T.geometry(H, W, self.max_stride, levels)
        return hit

    def forward_augment(self, im: torch.Tensor):
        """DetectionModel._predict_augment (nn/tasks.py:354-370) -> (y, None): three forwards at the scaled sizes, the scaled inputs
        made by bsy_scale_img, the passes clipped / descaled / concatenated by ONE bsy_tta_merge on the current stream.  A Segment
        graph (an OBB one, a pose one, a classification one) returns its single-scale forward, as the reference reverts for every class but
        DetectionModel (:356-358)."""
        if self.end2end:  # tasks.py:356: the reference does not augment an end2end model; its rows are no input of the merge
            raise NotImplementedError("test-time augmentation of an end2end (v10Detect) model is not accelerated (tasks.py:356)")
        with self._lock:
            if self.meta["nm"] or self.meta["ne"] or self.meta.get("nk", 0) or self.task == "classify":
                return self.forward(im)
            if im.device != self.device:
                raise ValueError(f"input on {im.device}, engine on {self.device}")
            if im.dtype not in (torch.float16, torch.float32) or im.dim() != 4 or im.shape[1] != 3:
                raise TypeError("input must be a BCHW fp16 or fp32 image tensor")
            im = self._dense(im)
            B, _, H, W = im.shape
            passes = self.tta_geometry(H, W)
            cur = torch.cuda.current_stream(self.device)
            if self._last_done is not None and self._last_stream != cur.cuda_stream:
                cur.wait_event(self._last_done)  # the scaled-input buffers may still be read by a forward on another stream
            # every scaled input first, back to back: the second resize finds the image still in the cache, not behind a forward
            xs = []
            for i, p in enumerate(passes):
                xi = im
                if p.ratio != 1.0 or p.flip:
                    # persistent per pass and shape: graph mode keys its captures by the input pointer (and no allocator churn)
                    key = (i, B, p.padded[0], p.padded[1], im.dtype)
                    buf = self._tta_bufs.get(key)
                    if buf is None:
                        while len(self._tta_bufs) >= 3 * max(self.max_plans, 1):  # rect batches: bounded like the plans
                            self._tta_bufs.popitem(last=False)
                        buf = self._tta_bufs[key] = torch.empty((B, 3) + p.padded, dtype=im.dtype, device=self.device)
                    self._tta_bufs.move_to_end(key)
                    xi = O.scale_img(im, p.ratio, p.flip, self.max_stride, out=buf)
                xs.append(xi)
            ys = []
            for xi in xs:
                y, _ = self.forward(xi, want_raw=False)
                if self.graph and len(passes) > self.graph_ring:
                    y = y.clone()  # a ring shorter than the pass count could hand out one slot twice
                ys.append(y)
            y = O.tta_merge(ys, [p.window for p in passes], [p.ratio for p in passes], [p.flip for p in passes], (H, W))
            if self._last_done is None:
                self._last_done = torch.cuda.Event()
            self._last_done.record(cur)
            self._last_stream = cur.cuda_stream
            return y, None

    def profile(self, im: torch.Tensor):
        """Per-op device time (ms) of one forward, measured with HIP events on the current stream."""
        im = self._dense(im)
        B, _, H, W = im.shape
        plan, h = self.plan_for(B, H, W, im.dtype, im.dtype)
        # bound: every output of a classify plan; of the others the image and what every caller gets -- y, or an end2end plan's pre-top-k
        # tensor and rows -- alone (no raw map, proto or keypoint store is timed)
        outs = _outputs(plan, self.task == "classify", self.device, im.dtype)
        ext, n = _bind(plan, im, outs if self.task == "classify" else {o.name: outs[o.name] for o in plan.outputs.values() if not o.raw_only})
        ms = (C.c_float * len(plan.ops))()
        L.check(L.lib.bsy_plan_profile(h, ext, n, L.stream_ptr(self.device), ms))
        return [(o["name"], o["kind"], float(t)) for o, t in zip(plan.ops, ms)], plan

    def check_guards(self):
        """Test aid (engines created with BSY_PLAN_GUARD=<bytes> set): [(plan key, buffer index, byte offset, op names that
        write that buffer)] for every plan with a damaged guard band -- empty when no kernel stored out of bounds."""
        bad = []
        for key, (plan, h) in self._plans.items():
            b, off = C.c_int32(-1), C.c_int64(0)
            L.check(L.lib.bsy_plan_check_guards(h, C.byref(b), C.byref(off)))
            if b.value >= 0:
                writers = [o["name"] for o in plan.ops for k in ("dst", "res") if o.get(k) is not None and getattr(o[k], "buf", -1) == b.value and k == "dst"]
                bad.append((key[:3], b.value, off.value, writers))
        return bad

    def read_view(self, plan, h, t) -> torch.Tensor:
        """Debug/test aid: copy an activation view back as a (B, C, H, W) fp32 CPU tensor."""
        hs, ws = (t.H // 2, t.W // 2) if t.up else (t.H, t.W)
        n = plan.B * hs * ws * t.ld
        host = torch.empty(n, dtype=torch.float32 if t.f32 else torch.float16)
        L.check(L.lib.bsy_plan_copy_buffer(h, t.buf, C.c_void_p(host.data_ptr()), n * host.element_size()))
        v = host.view(plan.B, hs, ws, t.ld)[..., t.coff:t.coff + t.C].permute(0, 3, 1, 2).float()
        return torch.nn.functional.interpolate(v, scale_factor=2.0, mode="nearest") if t.up else v.contiguous()

    def close(self):
        for _, h in self._plans.values():
            L.lib.bsy_plan_destroy(h)
        self._plans.clear()
        self._tta_bufs.clear()
        if self._h:
            L.lib.bsy_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
