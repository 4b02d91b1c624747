"""graph_helpers.check_y / check_raw on both sides of every bound the graph-family files pass them, on numpy arrays (no GPU, no engine).

EXPECTED restates each family's constants as numbers, so a bound changes in two visible places or this file fails.  The toy layout: two
images, nc = 2, a 2 x 2 level at stride 8 (box bound 1 px) and a 1 x 1 level at stride 64 (2 px).  The reference is zero where an error
is planted, so the error the checker measures is the planted value to the bit, and "just inside" / "just outside" are the bound itself
and its floating-point neighbour: a strict bound refuses the bound and admits the value below it, a non-strict one admits the bound and
refuses the value above it."""
import importlib
import math

import numpy as np
import pytest

from graph_helpers import RawBounds, YBounds, check_raw, check_y, level_of_anchor

Y = YBounds(score16=1e-2, p999_16=None, box16=1.0, score32=1e-3, box32=1e-3)
RAW = RawBounds(rel16=3e-2, strict16=False, floor16=True, rel32=1e-3)  # e <= 3e-2 * max(1, mx)
MAP = RawBounds(rel16=2e-2, strict16=True, floor16=False, rel32=1e-3)  # e < 2e-2 * mx
EXPECTED = {
    "test_ghost": {"Y_BOUNDS": Y, "RAW_BOUNDS": RAW},
    "test_yolov3": {"Y_BOUNDS": Y, "RAW_BOUNDS": RAW},
    "test_yolov10": {"Y_BOUNDS": Y, "RAW_BOUNDS": RAW},
    "test_world": {"Y_BOUNDS": Y, "RAW_BOUNDS": RAW},
    "test_p2p6": {"Y_BOUNDS": Y, "RAW_BOUNDS": RAW, "MASK_BOUNDS": MAP},
    "test_yolov6": {"Y_BOUNDS": Y._replace(p999_16=5e-3), "RAW_BOUNDS": RawBounds(rel16=1e-2, strict16=False, floor16=False, rel32=1e-3)},  # e <= 1e-2 * mx
    "test_yolov9": {"Y_BOUNDS": Y, "MAP_BOUNDS": MAP},
    "test_yolov9e": {"Y_BOUNDS": Y, "MAP_BOUNDS": MAP},
}
WHOLE_MAP = ("test_yolov9", "test_yolov9e")  # the families that hold the box to one bound over the whole map
FAMILIES = list(EXPECTED)
RAW_CONSTANTS = [(f, k) for f in FAMILIES for k in EXPECTED[f] if k != "Y_BOUNDS"]
NC, STRIDES, LEVELS, IMGSZ = 2, [8.0, 64.0], [(2, 2), (1, 1)], 192
LVL = level_of_anchor(LEVELS)
UP, DOWN = math.inf, -math.inf


def _constant(family, name):
    got = getattr(importlib.import_module(family), name)
    assert got == EXPECTED[family][name] and type(got) is type(EXPECTED[family][name]), (family, name, got)
    return got


def _next(v, towards):
    return float(np.nextafter(v, towards))


def _y(family, precision, score=0.0, box=None, bounds=None):
    """check_y of a reference with zeros where errors go: `score` added to every class score, box = (anchor, error) planted in one
    coordinate of one image."""
    ref = np.random.default_rng(0).standard_normal((2, 4 + NC, len(LVL)))
    ref[:, 4:] = 0.0
    y = ref.copy()
    y[:, 4:] += score
    if box is not None:
        ref[1, 2, box[0]] = 0.0
        y[1, 2, box[0]] = box[1]
    per_level = family not in WHOLE_MAP
    check_y(y, ref, STRIDES if per_level else None, LVL if per_level else None, IMGSZ, precision, family, NC, bounds or _constant(family, "Y_BOUNDS"))


def _refused(match, *args, **kw):
    with pytest.raises(AssertionError, match=match):
        _y(*args, **kw)


@pytest.mark.parametrize("family", FAMILIES)
def test_check_y_fp16(family):
    b = _constant(family, "Y_BOUNDS")
    _y(family, "fp16")
    p999 = b.p999_16 if b.p999_16 is not None else b.score16  # the largest uniform score error: every quantile of it is the value
    _y(family, "fp16", score=_next(p999, DOWN))
    _refused("score" if b.p999_16 is None else "p99.9", family, "fp16", score=p999)  # (with a percentile bound: the maximum is inside its own)
    # the maximum alone, one score off and the others exact: of 20 errors the 99.9th percentile lies 0.981 of the way from the second
    # largest to the largest, so this is run without the percentile bound, and with it the percentile is what refuses the inside case
    ref = np.zeros((2, 4 + NC, len(LVL)))
    y = ref.copy()
    for at, ok in ((_next(b.score16, DOWN), True), (b.score16, False)):
        y[0, 4 + 1, 3] = at
        for bounds in (b._replace(p999_16=None), b):
            if ok and bounds.p999_16 is None:
                check_y(y, ref, STRIDES, LVL, IMGSZ, "fp16", family, NC, bounds)
            else:
                with pytest.raises(AssertionError, match="score" if not ok else "p99.9"):
                    check_y(y, ref, STRIDES, LVL, IMGSZ, "fp16", family, NC, bounds)
    # boxes: 1 px on the stride-8 level; on the stride-64 level 2 px per level, 1 px over the whole map
    first, last = 1, len(LVL) - 1
    _y(family, "fp16", box=(first, _next(b.box16, DOWN)))
    _refused("box", family, "fp16", box=(first, b.box16))
    far = b.box16 if family in WHOLE_MAP else b.box16 * STRIDES[1] / 32.0
    assert far == (1.0 if family in WHOLE_MAP else 2.0)
    _y(family, "fp16", box=(last, _next(far, DOWN)))
    _refused("box", family, "fp16", box=(last, far))
    _y(family, "fp16", box=(first, -_next(b.box16, DOWN)))  # the error is a magnitude
    _refused("box", family, "fp16", box=(first, -b.box16))


@pytest.mark.parametrize("precision", ["fp32x", "fp32"])
@pytest.mark.parametrize("family", FAMILIES)
def test_check_y_fp32(family, precision):
    b = _constant(family, "Y_BOUNDS")
    _y(family, precision, score=b.score32)
    _refused("score", family, precision, score=_next(b.score32, UP))
    for anchor in (1, len(LVL) - 1):  # one bound for every level: a share of the image size
        _y(family, precision, box=(anchor, b.box32 * IMGSZ))
        _refused("box", family, precision, box=(anchor, _next(b.box32 * IMGSZ, UP)))
    assert b.box32 * IMGSZ < b.box16 and b.score32 < b.score16  # (so the fp16 cases above are no fp32 cases)


def _raw(bounds, precision, mx, e, shape=(2, 3, 2, 2)):
    ref = np.zeros(shape)
    ref[0, 0, 0, 0] = -mx  # the reference's largest magnitude, away from the planted error
    got = ref.copy()
    got[1, 2, 1, 1] = e
    check_raw(got, ref, precision, "raw", bounds)


@pytest.mark.parametrize("family,name", RAW_CONSTANTS)
def test_check_raw(family, name):
    b = _constant(family, name)
    for mx in (4.0, 0.5):  # above and below the floor of 1
        lim = b.rel16 * (max(1.0, mx) if b.floor16 else mx)
        inside, outside = (_next(lim, DOWN), lim) if b.strict16 else (lim, _next(lim, UP))
        _raw(b, "fp16", mx, inside)
        _raw(b, "fp16", mx, -inside)
        with pytest.raises(AssertionError):
            _raw(b, "fp16", mx, outside)
        for precision in ("fp32x", "fp32"):
            lim = b.rel32 * max(1.0, mx)
            _raw(b, precision, mx, lim)
            with pytest.raises(AssertionError):
                _raw(b, precision, mx, _next(lim, UP))
            with pytest.raises(AssertionError):
                _raw(b, precision, mx, inside)  # what fp16 storage is allowed is refused here
    for precision in ("fp16", "fp32"):
        with pytest.raises(AssertionError):  # a wrong shape, with no error at all
            check_raw(np.zeros((2, 3, 2, 2)), np.zeros((2, 3, 2, 1)), precision, "shape", b)
        with pytest.raises(AssertionError):  # ... one that broadcasts included
            check_raw(np.zeros((1, 3, 2, 2)), np.zeros((2, 3, 2, 2)), precision, "shape", b)


def test_the_checkers_print_their_figures_before_they_assert(capsys):
    with pytest.raises(AssertionError):
        _y("test_yolov6", "fp16", score=1.0)
    with pytest.raises(AssertionError):
        _raw(RAW, "fp16", 4.0, 1.0)
    out = capsys.readouterr().out
    assert "score max 1.00e+00 p99.9 1.00e+00 box per level ['0.00e+00', '0.00e+00']" in out and "err 1.00e+00 of max 4.000" in out
