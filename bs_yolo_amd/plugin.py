"""Reference-side installation: make an unmodified Ultralytics/BS-YOLO model dispatch its hot path to libbsyolo_hip.so.

Three hooks, each using an extension point the reference already has:

  accelerate(model)        whole-graph hook.  Rebinds ``model.forward`` on the instance -- the reference's own idiom
                           (``m.forward = m.forward_fuse``, nn/tasks.py:215) -- so that AutoBackend's in-memory branch
                           (nn/autobackend.py:136-147, call at :524) reaches the engine.  The graph comes from
                           ``model.yaml`` (the dict parse_model consumed, nn/tasks.py:313-321) and the weights from
                           ``model.state_dict()``.  ``augment=True`` on a ``DetectionModel`` runs the engine's test-time
                           augmentation (tasks.py:354-370; ``tta="reference"`` opts out).  A ``ClassificationModel``
                           (tasks.py:439-490, a ``Classify`` head) returns ``(y, x)`` as Classify.forward does in eval (head.py:304).
                           A ``PoseModel`` (a ``Pose`` head) returns ``(y, (x_list, kpt))`` as Pose.forward does (head.py:250); with
                           the head's ``export`` flag set it keeps its own forward (kpts_decode's export branch, head.py:255-272).
                           A ``WorldModel`` of yolov8-worldv2.yaml (tasks.py:606-677; C2fAttn blocks, a ``WorldDetect`` head) runs with
                           ``model.txt_feats`` folded into the engine's weights; a call that passes ``txt_feats=`` keeps its own forward.
                           Anything else the engine does not cover
                           (training mode, visualize / embed / profile (tasks.py:137-164), augment on other model classes, CPU
                           tensors, unsupported modules) goes to the original forward.
  install(model)           per-module hook (the fallback level for graphs `accelerate` does not cover: a custom block, an
                           unknown head).  Rebinds ``forward`` on every ``Conv`` / ``DWConv`` INSTANCE (nn/modules/conv.py:133-151,
                           :224-229) -- again the reference's own idiom, ``m.forward = m.forward_fuse`` (nn/tasks.py:215) -- so
                           that the block modules' Python forwards (C2f, C3k, C2PSA, PMSFA ... call their child Convs) run
                           every convolution through ``bsy_conv2d`` / ``bsy_conv_first`` / ``bsy_dwconv``; and on the block
                           instances the library has an operator for: ``SPPF`` (block.py:3145-3149: ``bsy_sppf_pool`` on the
                           concat buffer), ``Attention`` (:4267-4286: ``bsy_attention`` + the ``pe`` depthwise conv with the
                           residual), ``Bottleneck`` / ``C3k2`` whose widths the fused kernels are built for (:3417-3419,
                           :3796-3804: ``bsy_bottleneck_fused`` / ``bsy_c3k2_fused``), ``Detect._inference``
                           (head.py:100-131: ``bsy_detect_decode``) and, on a ``Pose`` head, ``kpts_decode`` as well
                           (head.py:252-279: ``bsy_kpts_decode``).  Activations stay torch tensors in channels_last memory
                           format (= the kernels' NHWC, no copies); the rest (cat, chunk, upsample ...) stays with torch.
  install_nms(ops_module)  ``ultralytics.utils.ops.non_max_suppression`` is looked up as a module attribute on every
                           call (models/yolo/detect/predict.py:25, detect/val.py:95): replacing the attribute suffices.
  install_masks(ops_module) same for ``ultralytics.utils.ops.process_mask`` (models/yolo/segment/predict.py:53).
  install_val_metrics(v)   rebinds ``_process_batch`` on a Detection / Segmentation / OBB / Pose validator instance
                           (models/yolo/detect/val.py:209-228, segment/val.py:173-217, obb/val.py:53-80, pose/val.py:159-197):
                           true-positive matching on box IoU, mask IoU, probiou or keypoint similarity on the device.  On a
                           ClassificationValidator it rebinds ``update_metrics`` (classify/val.py:56-60): the top-5 rows come
                           from the forward's own launch, not from an argsort.
  install_preprocess(p)    rebinds ``BasePredictor.preprocess`` (engine/predictor.py:116-134) on a predictor instance so
                           lists of HWC BGR uint8 images are letterboxed on the device.
"""
from __future__ import annotations

import types
from typing import Optional

import torch

from . import lib as _L
from . import nms as _nms
from . import ops as _O
from .engine import YoloEngine, sppf_form
from .plan import Plan, qkv_perm
from .weights import BN_EPS, repconv_form

SUPPORTED_HEADS = ("Detect", "Segment", "OBB", "Classify", "Pose", "v10Detect", "WorldDetect")


def _on_device(t) -> bool:
    """The hooks' dispatch test: the library runs tensors that live on a ROCm device; everything else goes to the reference's own
    code.  One function so that the contract test (tests/test_host_logic.py, build container, no GPU) can let CPU tensors reach
    RECORDING stand-ins for the engine / NMS / letterbox calls while the reference's predictor drives the hooks -- the product never
    rebinds it, and the library itself has no CPU path (bs_yolo_amd.lib raises without the .so, YoloEngine without a GPU)."""
    return bool(t.is_cuda)


def _device_is_gpu(device) -> bool:
    return str(device).startswith("cuda")


def model_bn_eps(model) -> float:
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            return float(m.eps)
    return BN_EPS


def cfg_of(model) -> dict:
    """The yaml dict of a reference model (DetectionModel.yaml, nn/tasks.py:313) -- raises if the graph uses modules
    outside the accelerated set, so callers can fall back."""
    cfg = getattr(model, "yaml", None)
    if not isinstance(cfg, dict) or "backbone" not in cfg or "head" not in cfg:
        raise NotImplementedError("model has no yaml graph description")
    try:
        Plan(cfg, 1, 64, 64)  # raises NotImplementedError / AssertionError on unsupported graphs
    except NotImplementedError:
        # widths only the fp32 modes take (BS-YOLO's PMSFA on a width that is not a multiple of 8, e.g. a width multiple of 0.1875): fp32
        # callers still get the engine, fp16 calls fall back to the reference forward when their engine is built
        Plan(cfg, 1, 64, 64, precision="fp32")
    return cfg


def _weights_version(model) -> tuple:
    """Cheap fingerprint of the parameters and buffers: in-place updates (optimizer steps, EMA, load_state_dict's copy_)
    bump ``Tensor._version``; ``.half()`` / ``.to()`` / ``fuse()`` replace the storages (data_ptr).  Inference tensors
    -- what ``fuse()`` creates under the predictor's / validator's ``smart_inference_mode`` (engine/predictor.py:219,
    engine/validator.py:105) -- carry no version counter (reading it raises) and cannot be updated in place outside
    inference mode, so their storage pointer is the whole fingerprint."""
    n, ver, ptr = 0, 0, 0
    for t in list(model.parameters()) + list(model.buffers()):
        n += 1
        try:  # (`is_inference()` alone does not tell: a Parameter whose .data was swapped by .half() / .to() outside inference
            ver += t._version  # mode reports False and still has no counter)
        except RuntimeError:
            pass
        ptr ^= t.data_ptr() + 0x9E3779B1 * n
    return (n, ver, ptr)


def _graph_facts(cfg: dict):
    """(graph_support(cfg), max_stride(cfg)) from one plan per precision."""
    out, gs = {}, 0
    for prec in ("fp16", "fp32"):
        try:
            gs = int(max(Plan(cfg, 1, 64, 64, precision=prec).meta["strides"]))  # the same in every precision that builds
            out[prec] = True
        except (NotImplementedError, AssertionError):
            out[prec] = False
    return out, gs


def graph_support(cfg: dict) -> dict:
    """Which engine precisions can run this yaml graph: {"fp16": bool, "fp32": bool} (the fp32 / fp32x modes also take PMSFA widths
    that are not multiples of 8 channels, e.g. BS-YOLO at a width multiple of 0.1875).  Decided once, on the host, from the plan alone."""
    return _graph_facts(cfg)[0]


def max_stride(cfg: dict) -> int:
    """int(max(model.stride)) of a yaml graph (32; 64 with a P6 head): what the engine's inputs must be multiples of.  Raises
    NotImplementedError for a graph no precision can run."""
    gs = _graph_facts(cfg)[1]
    if not gs:
        raise NotImplementedError("the graph is not on the accelerated path in any precision")
    return gs


def _head_attr(model, attr: str, default):
    """`attr` of the last layer of a reference model (BaseModel.model, an nn.Sequential), `default` where there is none."""
    seq = getattr(model, "model", None)
    kids = list(seq.children()) if isinstance(seq, torch.nn.Module) else []
    return getattr(kids[-1], attr, default) if kids else default


def _head_exports(model) -> bool:
    """Whether the last layer of a reference model has its `export` flag set."""
    return bool(_head_attr(model, "export", False))


_ACT_IDS = ((torch.nn.ReLU, _L.ACT_RELU), (torch.nn.SiLU, _L.ACT_SILU), (torch.nn.Identity, _L.ACT_NONE))


def _check_acts(model, cfg: dict, sppf_act: str, support: dict) -> None:
    """Every conv the plan runs with an activation id (CONV_FIRST / FIRST_POOL / STEM / CONV ops over a Conv module's record) against the
    live module's `act`: nn.ReLU <-> 2, nn.SiLU <-> 1, nn.Identity <-> 0.  A mismatch -- a module whose activation was swapped after the
    yaml built it -- raises NotImplementedError: the engine would compute another function than the model.  Modules the plan's names
    do not resolve to, and (outside ReLU graphs) activations of other classes, are left as they always were.
    Cost and reach: this builds one whole Plan at 64 x 64 (host-side flattening, a few milliseconds) at accelerate() and again at every
    engine rebuild, only to walk its op names; and it walks ONE precision's plan -- fp16 where the graph has one, else fp32 -- so a
    module is checked under the name that precision's fusions give it (the stem and the fused head exist in fp16 alone).  Every Conv
    module appears in both precisions' plans with the same activation, so one walk covers them."""
    relu = cfg.get("activation") == "nn.ReLU()"
    plan = Plan(cfg, 1, 64, 64, precision="fp16" if support.get("fp16") else "fp32", sppf_act=sppf_act)
    for o in plan.ops:
        if o["kind"] not in (_L.OP_CONV_FIRST, _L.OP_FIRST_POOL, _L.OP_STEM, _L.OP_CONV):
            continue
        for key in ("wkey", "wkey2") if o["kind"] in (_L.OP_STEM, _L.OP_CONV) else ("wkey",):
            r = plan.wrecs.get(o.get(key))
            if r is None or r.kind not in ("conv", "first", "first_s2d") or (key == "wkey2" and o["kind"] == _L.OP_CONV):
                continue
            try:
                act = model.get_submodule(r.name).act
            except AttributeError:
                continue
            ids = [i for cls, i in _ACT_IDS if isinstance(act, cls)]
            if (ids and ids[0] != o["act"]) or (relu and not ids):
                raise NotImplementedError(f"{r.name}: the module's activation is {act}, the plan runs act = {o['act']} there "
                                          "(0 identity, 1 SiLU, 2 ReLU): the model does not compute what its yaml describes")


FP32_MODES = {"engine_fp32x": "fp32x", "engine_fp32": "fp32", "engine": "fp16", "reference": None}


def accelerate(model, device: Optional[int] = None, verbose: bool = False, fp32_inputs: Optional[str] = None,
               tta: Optional[str] = None, e2e_raw: bool = True):
    """Install the engine behind ``model.forward``.  Returns the same model object.

    fp32_inputs: what an fp32 image tensor gets (the reference's ``predict()`` default is ``half=False``,
    engine/predictor.py:131).  The product path stores activations in fp16, which is NOT the fp32 model's arithmetic
    (max |dscore| up to 6e-3 against the fp32 reference, vs the north-star's 1e-3), so it is never
    applied to fp32 callers silently:
      ``"engine_fp32x"`` (default) the engine's fp32x mode: fp32 storage, dense convs on the fp16 matrix pipe with both operands
                                   split into f16 pairs (csrc/conv32x_mfma.hip; |dscore| ~1e-5, |dbox| ~1e-5 * imgsz against the
                                   fp32 reference -- the north-star's 1e-3 with two orders of margin -- at 2-3x the exact mode's
                                   throughput; a one-time log line says which mode runs);
      ``"engine_fp32"``            the exact fp32 mode: convs on the fp32 matrix pipe (csrc/conv32_mfma.hip: exact f32 products,
                                   k-ordered f32 sums, bit-reproducible against the scalar kernels);
      ``"engine"``                 opt in to the fast fp16-storage path for fp32 inputs (outputs come back as fp32);
      ``"reference"``              leave fp32 inputs to the original forward.
    ``BSY_FP32_INPUTS`` overrides the default.  fp16 inputs (``half=True`` / ``model.half()``) always run on the fp16
    engine: there the reference itself computes in fp16.

    Graphs only some precisions can run (``graph_support``): calls in a precision the engine does not take go straight to the
    reference forward -- decided here, once, not by a failing engine build on every call.

    tta: what ``augment=True`` (test-time augmentation, nn/tasks.py:354-370) gets on a ``DetectionModel``: ``"engine"`` (default)
    the engine's three scaled passes + HIP glue (YoloEngine.forward_augment), in whichever precision the call runs;
    ``"reference"`` the original forward.  ``BSY_TTA`` overrides the default; ``state["tta_calls"]`` counts engine TTA calls.

    A YOLOv10 model (a ``v10Detect`` head) returns the engine's pair ``(rows, {"one2many": [...], "one2one": [...]})``, the reference's
    own return value in eval (head.py:96-98); ``max_det`` is read from the head (``model.model[-1].max_det``) when the engine is built.
    e2e_raw: True (default) keeps the raw maps of both head copies in that dict -- the validator's loss reads them during training --;
    False runs the rows-only plan, without the one2many branches, and the dict holds ``None`` for every level.  ``augment=True`` (the
    reference does not augment an end2end model, tasks.py:356) and a head with ``export`` set keep their own forward.

    A YOLO-World v2 model (a ``WorldDetect`` head) returns ``(y, raws)`` as WorldDetect.forward does in eval, scored against
    ``model.txt_feats`` as it is at the call: the engine's key fingerprints that tensor (storage, version counter, shape), so
    ``set_classes`` (a new tensor, maybe a new row count: a new plan) or an in-place edit rebuilds the engine, counted in
    ``state["rebuilds"]``.  A call with a ``txt_feats=`` keyword (per-call text, tasks.py:651) and ``augment=True`` (the class is not
    ``DetectionModel``) keep their own forward."""
    import os
    cfg = cfg_of(model)
    support, gs = _graph_facts(cfg)  # gs: a P6 graph takes multiples of 64; anything else goes to the reference forward, as non-multiples of 32 do
    orig_forward = model.forward
    classify = cfg["head"][-1][2] == "Classify"
    pose = cfg["head"][-1][2] == "Pose"
    e2e = cfg["head"][-1][2] == "v10Detect"
    world = cfg["head"][-1][2] == "WorldDetect"
    state = {"engine": None, "engine32": None, "key": None, "fallbacks": 0, "engine_calls": 0, "fp32_calls": 0, "rebuilds": 0,
             "tta_calls": 0, "support": support, "failed": set(), "repconv": None, "sppf_act": sppf_form(model, cfg)}
    _check_acts(model, cfg, state["sppf_act"], support)  # raises before anything is rebound: the model keeps its forward
    fp32_mode = fp32_inputs or os.environ.get("BSY_FP32_INPUTS", "engine_fp32x")
    if fp32_mode not in FP32_MODES:
        raise ValueError(f"fp32_inputs must be one of {sorted(FP32_MODES)}, not {fp32_mode!r}")
    prec32 = FP32_MODES[fp32_mode]  # engine precision fp32 images run in (None: the reference forward)
    tta_mode = tta or os.environ.get("BSY_TTA", "engine")
    if tta_mode not in ("engine", "reference"):
        raise ValueError(f"tta must be 'engine' or 'reference', not {tta_mode!r}")

    def _engine_for(dev: torch.device, precision: str = "fp16") -> YoloEngine:
        max_det = int(_head_attr(model, "max_det", 300)) if e2e else 300  # v10Detect.max_det (head.py:601), read at every build
        key = (dev.index or 0, _weights_version(model), max_det)
        txt = getattr(model, "txt_feats", None) if world else None
        if world:
            if not torch.is_tensor(txt):
                raise NotImplementedError("the model holds no txt_feats tensor: a YOLO-World graph is scored against it")
            try:
                ver = txt._version
            except RuntimeError:  # (an inference tensor: no counter, and no in-place edit outside inference mode)
                ver = -1
            key += ((txt.data_ptr(), ver, tuple(txt.shape)),)
        if state["key"] != key:
            for k in ("engine", "engine32"):
                if state[k] is not None:
                    state[k].close()
                    state[k] = None
            state["key"] = key
            state["failed"].clear()
        slot = "engine" if precision == "fp16" else "engine32"
        if state[slot] is None:
            # weights are read at this moment: after AutoBackend has called fuse()/half() (autobackend.py:139-145); the key
            # makes a later in-place update (EMA, load_state_dict, a training step) or a .half()/.to() rebuild the engine
            sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
            state["rebuilds"] += 1
            # YOLOv9: the fork's own RepConv or upstream's (an upstream-pickled checkpoint), told apart by the keys -- at every build,
            # so a rebuild after a weight reload or a fuse() sees the form the model holds now
            state["repconv"] = repconv_form(sd)
            # YOLOv6: SPPF's activation, read off the live module like the RepConv form (Plan.sppf_act)
            state["sppf_act"] = sppf_form(model, cfg)
            # ... and the modules' activations against the plan's ids again: one swapped since accelerate() (the weights' fingerprint
            # does not see it, so this holds from the next rebuild on) sends the call to the reference forward, which computes it
            _check_acts(model, cfg, state["sppf_act"], support)
            state[slot] = YoloEngine(cfg, sd, device=dev.index or 0, bn_eps=model_bn_eps(model), precision=precision,
                                     repconv=state["repconv"], max_det=max_det, sppf_act=state["sppf_act"],
                                     txt_feats=txt.detach().float().cpu() if world else None)
        return state[slot]

    def forward(self, x, *args, **kwargs):
        augment = kwargs.get("augment", False)
        visualize = kwargs.get("visualize", False)
        embed = kwargs.get("embed", None)
        profile = kwargs.get("profile", False)
        # augment=True: the engine's TTA for exactly the class the reference runs it for (tasks.py:356-358: DetectionModel, not
        # end2end), and then visualize / embed / profile are ignored as predict() does (tasks.py:134-136); anything else keeps its
        # own forward (which reverts to single-scale or augments in torch)
        if augment:
            if tta_mode != "engine" or type(self).__name__ != "DetectionModel" or getattr(self, "end2end", False) or e2e:
                state["fallbacks"] += 1
                return orig_forward(x, *args, **kwargs)
            visualize = embed = profile = False
        # Classify.export (head.py:285, :304): y alone, the exporter's business; Pose.export (head.py:250, :255-272): y alone, and
        # kpts_decode's export branch is other arithmetic
        # v10Detect.export (head.py:98): the rows alone
        if (classify or pose or e2e) and _head_exports(self):
            state["fallbacks"] += 1
            return orig_forward(x, *args, **kwargs)
        if world and kwargs.get("txt_feats") is not None:  # per-call text (tasks.py:651): the engine's is folded into its weights
            state["fallbacks"] += 1
            return orig_forward(x, *args, **kwargs)
        if (self.training or visualize or embed or profile or args or not isinstance(x, torch.Tensor)
                or not _on_device(x) or x.dim() != 4 or x.dtype not in (torch.float16, torch.float32)
                or x.shape[1] != 3 or x.shape[2] % gs or x.shape[3] % gs or x.shape[0] == 0):
            state["fallbacks"] += 1
            return orig_forward(x, *args, **kwargs)
        precision = "fp16" if x.dtype == torch.float16 else prec32
        # a precision this graph cannot run in (or whose engine build has already failed for these weights): the reference runs it,
        # without another device-to-host weight copy + engine create / destroy per call
        if precision is None or not support["fp16" if precision == "fp16" else "fp32"] or precision in state["failed"]:
            state["fallbacks"] += 1
            return orig_forward(x, *args, **kwargs)
        want32 = precision != "fp16"
        if x.dtype == torch.float32 and not state.get("fp32_notice"):
            state["fp32_notice"] = True  # once per model: which engine default callers (predict(half=False)) are on, and the way out
            import logging
            logging.getLogger("bs_yolo_amd").warning(
                "fp32 images run in the engine's %s mode (%s).  fp32_inputs / BSY_FP32_INPUTS selects: engine_fp32x (default: fp32 storage, "
                "split-f16 matrix products, |dscore| ~1e-5 vs the fp32 model), engine_fp32 (exact fp32 arithmetic, 2-3x slower), engine "
                "(the fp16 product path, ~3x faster again, |dscore| up to 6e-3), reference (the original forward); predict(half=True) "
                "runs the fp16 path.", precision, fp32_mode)
        try:
            y, raws = _engine_for(x.device, precision)(x, augment=bool(augment), want_raw=bool(e2e_raw) or not e2e)
        except (_L.BsyError, NotImplementedError, AssertionError) as e:  # a shape / graph the engine rejects: the reference runs it
            if verbose:
                print(f"bs_yolo_amd: falling back to the reference forward ({e})")
            if state["engine" if precision == "fp16" else "engine32"] is None:
                state["failed"].add(precision)  # the BUILD failed: do not try again until the weights change
            state["fallbacks"] += 1
            return orig_forward(x, *args, **kwargs)
        state["fp32_calls" if want32 else "engine_calls"] += 1
        if augment:
            state["tta_calls"] += 1
        eng = state["engine32" if want32 else "engine"]
        if eng.task == "classify":
            # the top-k index rows of the same launch travel with y: ClassificationValidator.postprocess hands preds[0] on as it is
            # (classify/val.py:96-98), and install_val_metrics' update_metrics takes them instead of an argsort
            y._bsy_topk = eng.last_topk[0]
        return y, raws

    model.forward = types.MethodType(forward, model)
    model._bsy_state = state
    model._bsy_orig_forward = orig_forward
    return model


def restore(model):
    if hasattr(model, "_bsy_orig_forward"):
        model.forward = model._bsy_orig_forward
        st = model._bsy_state
        for k in ("engine", "engine32"):
            if st.get(k) is not None:
                st[k].close()
        del model._bsy_orig_forward, model._bsy_state
    return model


# ---------------------------------------------------------------------------------------------------------------------
# per-module hook
# ---------------------------------------------------------------------------------------------------------------------
def _conv_spec(m):
    """(kind, k, s, act) if `m` is a reference Conv / DWConv instance the kernels cover, else None."""
    conv, act = getattr(m, "conv", None), getattr(m, "act", None)
    if not isinstance(conv, torch.nn.Conv2d) or act is None or type(m).__name__ not in ("Conv", "DWConv"):
        return None
    if isinstance(act, torch.nn.SiLU):
        a = 1
    elif isinstance(act, torch.nn.Identity):
        a = 0
    else:
        return None
    (kh, kw), (sh, sw), (ph, pw) = conv.kernel_size, conv.stride, conv.padding
    if kh != kw or sh != sw or conv.dilation != (1, 1) or (ph, pw) != (kh // 2, kw // 2) or conv.padding_mode != "zeros":
        return None
    c1, c2, g = conv.in_channels, conv.out_channels, conv.groups
    if g == 1 and kh in (1, 3) and sh in (1, 2) and c1 % 8 == 0 and c2 % 8 == 0:
        return ("conv", kh, sh, a)
    if g == 1 and c1 == 3 and (kh, sh) == (3, 2) and c2 % 8 == 0:
        return ("first", kh, sh, a)
    if g == c1 == c2 and kh % 2 == 1 and kh <= 31 and sh in (1, 2) and c1 % 8 == 0:
        return ("dw", kh, sh, a)
    return None


def _conv_forward(m, spec):
    """The replacement forward of one Conv / DWConv instance.  Falls back to the module's own forward for anything but a
    fp16 CUDA NCHW tensor in eval mode; re-packs its weights when they change (``Tensor._version`` / storage)."""
    kind, k, s, act = spec
    orig = m.forward
    st = {"ver": None, "dev": None, "w": None, "calls": 0, "fallbacks": 0}

    def fwd(self, x):
        if (not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float16 or x.dim() != 4 or self.training
                or x.shape[1] != self.conv.in_channels):
            st["fallbacks"] += 1
            return orig(x)
        ver = _weights_version(self)
        if st["ver"] != ver or st["dev"] != x.device:
            st["w"] = (_O.pack_dw_weight if kind == "dw" else _O.pack_conv_weight)(*_folded(self, orig), x.device)
            st["ver"], st["dev"] = ver, x.device
        B, _, H, W = x.shape
        c2 = self.conv.out_channels
        out = torch.empty((B, (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1, c2), dtype=torch.float16, device=x.device)
        with torch.cuda.device(x.device):
            if kind == "first":
                _O.conv_first(x.contiguous(), st["w"], None, k, s, act, out=out)
            elif kind == "conv":
                _O.conv2d_nhwc(_nhwc(x), *st["w"], c2, k, s, act, out=out)
            else:
                _O.dwconv_nhwc(_nhwc(x), st["w"], None, s, act, out=out)
        st["calls"] += 1
        return out.permute(0, 3, 1, 2)  # NCHW tensor in channels_last memory format

    return fwd, st


def _silu_conv(m, k=None, s=1, groups=1) -> bool:
    """`m` is a reference Conv (+BN) + SiLU module with a square k x k kernel (k None: any), stride s, "same" padding."""
    conv, act = getattr(m, "conv", None), getattr(m, "act", None)
    return (isinstance(conv, torch.nn.Conv2d) and isinstance(act, torch.nn.SiLU) and conv.groups == groups
            and conv.kernel_size[0] == conv.kernel_size[1] and (k is None or conv.kernel_size[0] == k)
            and conv.stride == (s, s) and conv.padding == (conv.kernel_size[0] // 2,) * 2 and conv.dilation == (1, 1))


def _folded(m, forward=None):
    """(weight, bias) fp32 of a reference Conv module.  Un-fused (its forward = conv -> bn -> act) BatchNorm is folded in; after
    BaseModel.fuse() (tasks.py:209-215: conv replaced by the fused conv, `bn` deleted, forward = forward_fuse) conv.bias already
    holds it.  `forward`: the module's own forward where a hook has taken its place (captured at install time)."""
    from .weights import fold_conv_bn
    sd = {"m.conv." + n: t for n, t in m.conv.state_dict().items()}
    bn = getattr(m, "bn", None)
    if isinstance(bn, torch.nn.BatchNorm2d) and getattr(forward or m.forward, "__name__", "") != "forward_fuse":
        sd.update({"m.bn." + n: t for n, t in bn.state_dict().items()})
    elif "m.conv.bias" not in sd:
        sd["m.conv.bias"] = torch.zeros(m.conv.out_channels)
    return fold_conv_bn(sd, "m", float(bn.eps) if isinstance(bn, torch.nn.BatchNorm2d) else BN_EPS)


def _block_spec(m):
    """Which block operator of the library covers `m` (a reference module instance), or None."""
    from . import lib as L
    name = type(m).__name__
    if name == "SPPF":
        pool = getattr(m, "m", None)
        if (isinstance(pool, torch.nn.MaxPool2d) and pool.kernel_size == 5 and pool.stride == 1 and pool.padding == 2
                and _silu_conv(getattr(m, "cv1", None), 1) and _silu_conv(getattr(m, "cv2", None), 1)
                and m.cv1.conv.out_channels % 8 == 0 and m.cv2.conv.in_channels == 4 * m.cv1.conv.out_channels):
            return "sppf"
    if name == "Attention":
        if (all(hasattr(m, a) for a in ("qkv", "proj", "pe", "num_heads", "key_dim", "head_dim", "scale"))
                and m.key_dim == 32 and m.head_dim == 64 and _conv_spec(m.qkv) == ("conv", 1, 1, 0) and _conv_spec(m.proj) == ("conv", 1, 1, 0)
                and _conv_spec(m.pe) == ("dw", 3, 1, 0)):
            return "attention"
    if name == "Bottleneck":
        cv1, cv2 = getattr(m, "cv1", None), getattr(m, "cv2", None)
        if (getattr(m, "add", False) and _silu_conv(cv1, 3) and _silu_conv(cv2, 3)
                and L.lib.bsy_bottleneck_fused_supported(cv1.conv.in_channels, cv1.conv.out_channels) == 1):
            return "bottleneck"
    if name in ("C3k2", "C2f"):
        mm = getattr(m, "m", None)
        if (isinstance(mm, torch.nn.ModuleList) and len(mm) == 1 and type(mm[0]).__name__ == "Bottleneck" and getattr(mm[0], "add", False)
                and _silu_conv(getattr(m, "cv1", None), 1) and _silu_conv(getattr(m, "cv2", None), 1)
                and _silu_conv(mm[0].cv1, 3) and _silu_conv(mm[0].cv2, 3) and mm[0].cv1.conv.out_channels * 2 == m.c
                and L.lib.bsy_c3k2_fused_supported(m.cv1.conv.in_channels, m.c, m.cv2.conv.out_channels) == 1):
            return "c3k2"
    if name in ("Detect", "Segment"):
        if (getattr(m, "reg_max", 0) == 16 and 1 <= getattr(m, "nl", 0) <= _L.BSY_MAX_LEVELS and not getattr(m, "export", False)
                and getattr(m, "format", None) is None and hasattr(m, "_inference")):
            return "detect"
    if name == "Pose":  # Detect's condition plus a keypoint shape bsy_kpts_decode takes (head.py:230-279)
        ks = getattr(m, "kpt_shape", None)
        if (getattr(m, "reg_max", 0) == 16 and 1 <= getattr(m, "nl", 0) <= _L.BSY_MAX_LEVELS and not getattr(m, "export", False)
                and getattr(m, "format", None) is None and hasattr(m, "_inference") and hasattr(m, "kpts_decode")
                and isinstance(ks, (tuple, list)) and len(ks) == 2 and ks[1] in (2, 3) and 1 <= ks[0] <= 64):
            return "pose"
    return None


def _nhwc(x):
    """NCHW fp16 tensor -> its NHWC view (no copy when the tensor is already in channels_last memory format)."""
    return x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)


def _fp16_map(self, x, cin) -> bool:
    """What the block operators take: an fp16 NCHW device tensor of `cin` channels, in eval mode."""
    return torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float16 and x.dim() == 4 and not self.training and x.shape[1] == cin


def _pack_convs(dev, *convs):
    return [_O.pack_conv_weight(*_folded(c), dev) for c in convs]


def _sppf(self, x, pk, st):
    xn = _nhwc(x)
    B, H, W, _ = xn.shape
    c_, c2 = self.cv1.conv.out_channels, self.cv2.conv.out_channels
    cat = torch.empty((B, H, W, 4 * c_), dtype=torch.float16, device=x.device)
    out = torch.empty((B, H, W, c2), dtype=torch.float16, device=x.device)
    # cv1 writes channels [0, c_) of the concat buffer, the pools fill the rest in place, cv2 reads all of it
    _O.conv2d_nhwc(xn, *pk[0], c_, 1, 1, True, out=cat[..., :c_])
    _O.sppf_pool_nhwc(cat[..., :c_], out=cat)
    return _O.conv2d_nhwc(cat, *pk[1], c2, 1, 1, True, out=out).permute(0, 3, 1, 2)


def _pack_attention(self, dev):
    perm = torch.tensor(qkv_perm(self.num_heads, self.key_dim, self.head_dim))
    wq, bq = _folded(self.qkv)
    return [_O.pack_conv_weight(wq[perm], bq[perm], dev), *_pack_convs(dev, self.proj), _O.pack_dw_weight(*_folded(self.pe), dev)]


def _attention(self, x, pk, st):
    xn = _nhwc(x)
    B, H, W, c = xn.shape
    nh, kd, hd = self.num_heads, self.key_dim, self.head_dim
    ld = nh * (2 * kd + hd)
    qkv = torch.empty((B, H, W, ld), dtype=torch.float16, device=x.device)
    out = torch.empty((B, H, W, c), dtype=torch.float16, device=x.device)
    _O.conv2d_nhwc(xn, *pk[0], ld, 1, 1, False, out=qkv)
    att = _O.attention_nhwc(qkv.view(B, H * W, ld), nh, kd, hd, self.scale).view(B, H, W, c)
    xo = _O.dwconv3x3_nhwc(qkv[..., 2 * nh * kd:], pk[2], act=False, res=att)  # v @ attn^T + pe(v): the depthwise conv reads the v slice
    return _O.conv2d_nhwc(xo, *pk[1], c, 1, 1, False, out=out).permute(0, 3, 1, 2)


def _detect_takes(self, x) -> bool:
    """Detect._inference(x) with x = the per-level (B, 64 + nc, h, w) logit maps (head.py:100-131).  export / format / end2end variants
    compute something else (head.py:66-67, 109-127: dist2bbox(xywh=not end2end), format-specific rescaling), checked at CALL time:
    exporters flip these attributes on live modules."""
    xs = list(x) if isinstance(x, (list, tuple)) else None
    return not (xs is None or len(xs) != self.nl or self.training or getattr(self, "export", False) or getattr(self, "end2end", False)
                or getattr(self, "format", None) is not None
                or not all(torch.is_tensor(t) and t.is_cuda and t.dtype in (torch.float16, torch.float32) and t.dim() == 4
                           and t.shape[1] == self.no and t.shape[0] == xs[0].shape[0] for t in xs))


def _detect(self, x, pk, st):
    maps = [t.permute(0, 2, 3, 1).float().contiguous() for t in x]  # (B, h, w, no) f32: what bsy_detect_decode reads
    ld = self.no + (-self.no % 4)  # its rows are multiples of 4 floats: a one-class head (a stock pose model: no = 65) is padded
    if ld != self.no:
        maps = [torch.nn.functional.pad(t, (0, ld - self.no)) for t in maps]
    hw, strides = [(int(t.shape[1]), int(t.shape[2])) for t in maps], [float(v) for v in self.stride]
    y = _O.detect_decode([t[..., :64] for t in maps], [t[..., 64:] for t in maps], hw, strides, self.nc, x[0].dtype)
    st["levels"] = (hw, strides, y.shape[2], y.shape[0])
    # the reference's _inference caches anchors / strides per input shape as a side effect (head.py:105-107) and code outside
    # the path may read them (exporters, Detect.decode_bboxes callers): keep `shape` as the reference does and drop the cached
    # grids, so that the reference's own _inference -- on a fallback call -- rebuilds them for ITS shape instead of reusing ours
    self.shape = None
    return y


# kind -> (takes(self, x): the call is the operator's, checked at call time; pack(self, dev) -> device weights, or None; body(self, x,
# weights, st) -> what the module's own method returns)
_BLOCKS = {
    "sppf": (lambda self, x: _fp16_map(self, x, self.cv1.conv.in_channels), lambda self, dev: _pack_convs(dev, self.cv1, self.cv2), _sppf),
    "attention": (lambda self, x: _fp16_map(self, x, self.num_heads * self.head_dim), _pack_attention, _attention),
    "bottleneck": (lambda self, x: _fp16_map(self, x, self.cv1.conv.in_channels), lambda self, dev: _pack_convs(dev, self.cv1, self.cv2),
                   lambda self, x, pk, st: _O.bottleneck_fused(_nhwc(x), pk[0], None, pk[1], None).permute(0, 3, 1, 2)),
    "c3k2": (lambda self, x: _fp16_map(self, x, self.cv1.conv.in_channels),
             lambda self, dev: _pack_convs(dev, self.cv1, self.m[0].cv1, self.m[0].cv2, self.cv2),
             lambda self, x, pk, st: _O.c3k2_fused(_nhwc(x), pk[0], None, pk[1], None, pk[2], None, pk[3], None).permute(0, 3, 1, 2)),
    "detect": (_detect_takes, None, _detect),
    "pose": (_detect_takes, None, _detect),
}


def _block_forward(m, kind):
    """The replacement `forward` (`_inference` for Detect and Pose) of one block instance: one skeleton, the kind (_BLOCKS) says which
    calls it takes, how its weights pack and what it runs.  Anything it does not take reaches the module's own method.  Weights are
    re-packed when they change (`_weights_version`) or move to another device, never per call."""
    takes, pack, body = _BLOCKS[kind]
    attr = "_inference" if kind in ("detect", "pose") else "forward"
    orig = getattr(m, attr)
    # levels (detect / pose): what the last _inference call decoded -- ((h, w) per level, strides, A, B) -- or None when it fell back;
    # Pose's kpts_decode hook, which runs later in the same forward (head.py:246-249), reads it
    st = {"ver": None, "dev": None, "w": None, "calls": 0, "fallbacks": 0, "kind": kind, "attr": attr, "levels": None}

    def fwd(self, x):
        if not takes(self, x):
            st["fallbacks"] += 1
            st["levels"] = None
            return orig(x)
        dev = (x if torch.is_tensor(x) else x[0]).device
        if pack is not None:
            ver = _weights_version(self)
            if st["ver"] != ver or st["dev"] != dev:
                st["w"] = pack(self, dev)
                st["ver"], st["dev"] = ver, dev
        with torch.cuda.device(dev):
            y = body(self, x, st["w"], st)
        st["calls"] += 1
        return y
    return fwd, st


def _pose_kpts_forward(m, st):
    """The replacement `kpts_decode(bs, kpts)` of one Pose instance (head.py:252-279) whose `_inference` runs on the hook above (`st` is
    that hook's state).  The `_inference` hook never builds `self.anchors` (and resets `self.shape`), so this one reads the level sizes
    and strides that hook recorded for the same forward.  Whenever that call itself fell back the reference's anchors are valid, and the
    original method runs; it also runs on `export` (checked at call time), for CPU tensors and for a map that is not the recorded
    (B, nk, A)."""
    orig = m.kpts_decode

    def fwd(self, bs, kpts):
        lv = st["levels"]
        if (lv is None or getattr(self, "export", False) or not torch.is_tensor(kpts) or not kpts.is_cuda
                or kpts.dtype not in (torch.float16, torch.float32) or kpts.dim() != 3
                or tuple(kpts.shape) != (lv[3], self.kpt_shape[0] * self.kpt_shape[1], lv[2])):
            st["kpt_fallbacks"] = st.get("kpt_fallbacks", 0) + 1
            return orig(bs, kpts)
        with torch.cuda.device(kpts.device):
            y = _O.kpts_decode(kpts.contiguous(), lv[0], lv[1], self.kpt_shape)
        st["kpt_calls"] = st.get("kpt_calls", 0) + 1
        return y
    return fwd


def install(model, verbose: bool = False, blocks: bool = True) -> int:
    """Per-module hook: every covered Conv / DWConv instance of `model` runs its convolution in the HIP library, and (blocks=True)
    every SPPF / Attention / Detect instance -- and every Bottleneck / C3k2 whose widths the fused kernels are built for -- runs on
    the library's block operator (fp16 CUDA inputs in eval mode; anything else reaches the module's own method).  Returns the
    number of instances rebound; `uninstall(model)` undoes it.  Call it AFTER `model.fuse()` if the model is to be fused (fuse()
    rebinds `forward` itself).  Use `accelerate(model)` where the whole graph is covered -- it is 5-10x faster (all blocks fused,
    no per-layer Python); this is the level for graphs with modules the engine does not know."""
    n = 0
    for name, m in model.named_modules():
        if hasattr(m, "_bsy_conv") or hasattr(m, "_bsy_block"):
            continue
        spec = _conv_spec(m)
        if spec is not None:
            fwd, st = _conv_forward(m, spec)
            st["orig"] = m.__dict__.get("forward")  # an instance attribute (set by fuse()) or None (the class method)
            m._bsy_conv = st
            m.forward = types.MethodType(fwd, m)
            n += 1
            if verbose:
                print(f"bs_yolo_amd.install: {name} -> {spec}")
            continue
        kind = _block_spec(m) if blocks else None
        if kind is not None:
            fwd, st = _block_forward(m, kind)
            st["orig"] = m.__dict__.get(st["attr"])
            if kind == "pose":  # a second method of the same instance; uninstall restores the pairs of st["more"] as it does st["attr"]
                st["more"] = [("kpts_decode", m.__dict__.get("kpts_decode"))]
                m.kpts_decode = types.MethodType(_pose_kpts_forward(m, st), m)
            m._bsy_block = st
            setattr(m, st["attr"], types.MethodType(fwd, m))
            n += 1
            if verbose:
                print(f"bs_yolo_amd.install: {name} -> {kind}")
    return n


def uninstall(model) -> int:
    n = 0
    for m in model.modules():
        for key, attr in (("_bsy_conv", None), ("_bsy_block", None)):
            st = m.__dict__.pop(key, None)
            if st is None:
                continue
            for a, orig in [(st.get("attr", "forward"), st["orig"])] + st.get("more", []):
                if orig is None:
                    delattr(m, a)
                else:
                    setattr(m, a, orig)
            n += 1
    return n


def install_nms(ops_module, rotated: bool = False):
    """ops_module = ultralytics.utils.ops.  GPU tensors go to the HIP NMS; everything else to the original.
    rotated=True also takes the OBB calls (``rotated=True``, obb/predict.py:33-41) onto bsy_nms_rotated -- the working path for the
    fork, whose own rotated NMS raises NameError (utils/ops.py:14 leaves batch_probiou unimported); by default they stay on the
    original."""
    orig = ops_module.non_max_suppression
    if getattr(orig, "_bsy", False):
        if getattr(orig, "_bsy_rotated", False) == bool(rotated):
            return orig
        orig = orig._bsy_orig  # installed before with the other `rotated` choice: wrap the original again
    take_rotated = bool(rotated)

    def non_max_suppression(prediction, *args, **kwargs):
        p = prediction[0] if isinstance(prediction, (list, tuple)) else prediction
        # positional order after `prediction` (utils/ops.py:167-182): conf_thres, iou_thres, classes, agnostic, multi_label,
        # labels (5), max_det, nc, max_time_img, max_nms, max_wh, in_place, rotated (12)
        rotated = kwargs.get("rotated", False) or (len(args) > 12 and args[12])
        labels = kwargs.get("labels", ()) or (args[5] if len(args) > 5 else ())
        if (not isinstance(p, torch.Tensor)) or (not _on_device(p)) or (rotated and not take_rotated) \
                or (len(labels) and not rotated) or p.shape[-1] == 6 or p.dtype not in (torch.float16, torch.float32):
            return orig(prediction, *args, **kwargs)
        return _nms.non_max_suppression(prediction, *args, **kwargs)

    non_max_suppression._bsy = True
    non_max_suppression._bsy_rotated = take_rotated
    non_max_suppression._bsy_orig = orig
    ops_module.non_max_suppression = non_max_suppression
    return non_max_suppression


def install_masks(ops_module):
    """ops_module = ultralytics.utils.ops: GPU calls of process_mask (segment/predict.py:53) go to the HIP kernels."""
    from . import masks as _masks
    orig = ops_module.process_mask
    if getattr(orig, "_bsy", False):
        return orig

    def process_mask(protos, masks_in, bboxes, shape, upsample=False):
        if not (isinstance(protos, torch.Tensor) and protos.is_cuda):
            return orig(protos, masks_in, bboxes, shape, upsample)
        return _masks.process_mask(protos, masks_in, bboxes, shape, upsample)

    process_mask._bsy = True
    process_mask._bsy_orig = orig
    ops_module.process_mask = process_mask
    # the retina_masks path (segment/predict.py:48-50): process_mask_native and scale_masks (utils/ops.py:696-737)
    if hasattr(ops_module, "process_mask_native") and not getattr(ops_module.process_mask_native, "_bsy", False):
        orig_n = ops_module.process_mask_native

        def process_mask_native(protos, masks_in, bboxes, shape):
            if not (isinstance(protos, torch.Tensor) and protos.is_cuda):
                return orig_n(protos, masks_in, bboxes, shape)
            return _masks.process_mask_native(protos, masks_in, bboxes, shape)

        process_mask_native._bsy = True
        process_mask_native._bsy_orig = orig_n
        ops_module.process_mask_native = process_mask_native
    if hasattr(ops_module, "scale_masks") and not getattr(ops_module.scale_masks, "_bsy", False):
        orig_s = ops_module.scale_masks

        def scale_masks(masks, shape, padding=True):
            if not (isinstance(masks, torch.Tensor) and masks.is_cuda and masks.dim() == 4 and masks.dtype in (torch.float16, torch.float32)):
                return orig_s(masks, shape, padding)
            return _masks.scale_masks(masks, shape, padding)

        scale_masks._bsy = True
        scale_masks._bsy_orig = orig_s
        ops_module.scale_masks = scale_masks
    return process_mask


def install_val_metrics(validator):
    """validator = a ClassificationValidator: see _install_classify_metrics.  Else
    validator = a DetectionValidator, SegmentationValidator, OBBValidator or PoseValidator instance: its per-image `_process_batch`
    (models/yolo/detect/val.py:209-228, segment/val.py:173-217, obb/val.py:53-80, pose/val.py:159-197: an IoU matrix +
    match_predictions, numpy on the host in the reference) goes to the device kernels for CUDA detections.  The rebound method takes the segment validator's full
    signature and dispatches on the CALL, not on the class: masks=True -> mask IoU; masks false with both mask slots filled -> the
    PoseValidator's five-positional call (pose/val.py:140: predicted and label keypoints) -> keypoint similarity with the validator's
    `sigma`; 5-column labels (xywhr) -> probiou; everything else -> box IoU.  CPU tensors and more than 1024 detections go to the
    original method with the arguments they came with."""
    from . import val as _val
    if type(validator).__name__ == "ClassificationValidator":
        return _install_classify_metrics(validator)
    if not hasattr(validator, "_process_batch"):
        raise TypeError(f"install_val_metrics: {type(validator).__name__} is neither a ClassificationValidator nor a validator with _process_batch")
    orig = validator._process_batch

    def _process_batch(self, detections, gt_bboxes, gt_cls, pred_masks=None, gt_masks=None, overlap=False, masks=False):
        # the pose call (pose/val.py:140) is five positional arguments: its keypoints arrive in the two mask slots with masks=False
        kpts = not masks and pred_masks is not None and gt_masks is not None
        if not (isinstance(detections, torch.Tensor) and _on_device(detections)) or detections.shape[0] > 1024:
            if masks:
                return orig(detections, gt_bboxes, gt_cls, pred_masks, gt_masks, overlap, masks=True)
            if kpts:
                return orig(detections, gt_bboxes, gt_cls, pred_masks, gt_masks)
            return orig(detections, gt_bboxes, gt_cls)
        if masks:
            return _val.process_batch_masks(detections, gt_cls, pred_masks, gt_masks, overlap, self.iouv)
        if kpts:
            return _val.process_batch_kpts(detections, gt_bboxes, gt_cls, pred_masks, gt_masks, self.sigma, self.iouv)
        if gt_bboxes.dim() == 2 and gt_bboxes.shape[1] == 5:
            return _val.process_batch_rotated(detections, gt_bboxes, gt_cls, self.iouv)
        return _val.process_batch(detections, gt_bboxes, gt_cls, self.iouv)

    validator._process_batch = types.MethodType(_process_batch, validator)
    return validator


def _install_classify_metrics(validator):
    """validator = a ClassificationValidator instance (it has no `_process_batch`): `update_metrics(preds, batch)`
    (models/yolo/classify/val.py:56-60) appends preds.argsort(1, descending=True)[:, :min(nc, 5)] as int32 on the CPU.  For the y of an
    accelerated ClassificationModel -- a device tensor that carries the top-min(nc, 5) index rows bsy_classify_tail wrote in the same
    launch (accelerate's forward attaches them) -- those rows are appended instead: the same classes wherever the stored
    probabilities differ, the lower class first where they are equal (argsort leaves that order unspecified).  Any other `preds` (a CPU
    tensor, a device tensor of another model) goes to the original method.  The targets are handled as the reference does."""
    orig = validator.update_metrics

    def update_metrics(self, preds, batch):
        rows = getattr(preds, "_bsy_topk", None)
        n5 = min(len(self.names), 5)
        if not (isinstance(preds, torch.Tensor) and _on_device(preds)) or rows is None or tuple(rows.shape) != (preds.shape[0], n5):
            return orig(preds, batch)
        self.pred.append(rows.type(torch.int32).cpu())
        self.targets.append(batch["cls"].type(torch.int32).cpu())

    validator.update_metrics = types.MethodType(update_metrics, validator)
    return validator


def install_ap_per_class(metrics_module, device="cuda:0"):
    """metrics_module = ultralytics.utils.metrics: `ap_per_class` (:620-706, called by Metric / DetMetrics.process :940) goes
    to the device implementation when no plots are asked for (the plotting path stays the reference's own)."""
    from . import val as _val
    orig = metrics_module.ap_per_class
    if getattr(orig, "_bsy", False):
        return orig

    def ap_per_class(tp, conf, pred_cls, target_cls, plot=False, on_plot=None, save_dir=None, names={}, eps=1e-16, prefix=""):
        n = len(conf)
        if plot or not torch.cuda.is_available() or n == 0 or n > (1 << 20) or getattr(tp, "ndim", 2) != 2 or tp.shape[1] > 16:
            kw = dict(plot=plot, on_plot=on_plot, names=names, eps=eps, prefix=prefix)
            if save_dir is not None:
                kw["save_dir"] = save_dir
            return orig(tp, conf, pred_cls, target_cls, **kw)
        return _val.ap_per_class(tp, conf, pred_cls, target_cls, eps=eps, device=device)

    ap_per_class._bsy = True
    ap_per_class._bsy_orig = orig
    metrics_module.ap_per_class = ap_per_class
    return ap_per_class


def install_preprocess(predictor):
    """predictor = a BasePredictor instance whose model is already set up."""
    from . import letterbox as _lb
    orig = predictor.preprocess

    def preprocess(self, im):
        if isinstance(im, torch.Tensor) or not _device_is_gpu(self.device):
            return orig(im)
        return _lb.preprocess(list(im), tuple(self.imgsz), half=bool(self.model.fp16), pt=bool(self.model.pt),
                              stride=int(self.model.stride), device=str(self.device))

    predictor.preprocess = types.MethodType(preprocess, predictor)
    return predictor
