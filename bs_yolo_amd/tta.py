"""Test-time augmentation geometry: the host half of DetectionModel._predict_augment (nn/tasks.py:354-370).

Three passes -- scales (1, 0.83, 0.67), flips (none, left-right, none) -- each run by the engine at its padded size; the device
half is csrc/tta.hip (bsy_scale_img before a pass, ONE bsy_tta_merge after the last).  The sizes are scale_img's
(utils/torch_utils.py:430-442) and the anchor windows _clip_augmented's (:382-391), restated with the same Python float
expressions so that every pass runs at exactly the reference's shape.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

SCALES = (1, 0.83, 0.67)  # s = [1, 0.83, 0.67]  (tasks.py:361)
FLIPS = (None, 3, None)   # f = [None, 3, None]  (2 = up-down, 3 = left-right; tasks.py:362)


class Pass(NamedTuple):
    ratio: float
    flip: Optional[int]
    size: Tuple[int, int]    # resized (h, w) before the pad
    padded: Tuple[int, int]  # what the engine runs: multiples of gs
    window: Tuple[int, int]  # kept anchors [begin, end) of this pass's prediction


def scaled_size(h: int, w: int, ratio: float, gs: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """scale_img's resized and padded sizes; ratio 1.0 returns the input unchanged (torch_utils.py:432-433)."""
    if ratio == 1.0:
        return (h, w), (h, w)
    s = (int(h * ratio), int(w * ratio))
    return s, tuple(math.ceil(x * ratio / gs) * gs for x in (h, w))


def clip_windows(levels: Sequence[Sequence[Tuple[int, int]]]) -> List[Tuple[int, int]]:
    """_clip_augmented from each pass's detection levels [(h, w), ...] (largest map first, a plan's meta["levels"]): the first pass
    loses its last (coarsest) level, the last pass its first (finest); passes in between keep everything."""
    counts = [[lh * lw for lh, lw in lv] for lv in levels]
    wins = [(0, sum(c)) for c in counts]
    wins[0] = (0, sum(counts[0]) - counts[0][-1])
    wins[-1] = (counts[-1][0], sum(counts[-1]))
    return wins


def reference_windows(anchors: Sequence[int], nl: int) -> List[Tuple[int, int]]:
    """The reference's own formula (tasks.py:384-390: g = sum 4**x over nl levels, e = 1) on the passes' anchor counts."""
    g = sum(4 ** x for x in range(nl))
    wins = [(0, a) for a in anchors]
    i = (anchors[0] // g) * sum(4 ** x for x in range(1))
    wins[0] = (0, anchors[0] - i)
    i = (anchors[-1] // g) * sum(4 ** (nl - 1 - x) for x in range(1))
    wins[-1] = (i, anchors[-1])
    return wins


def geometry(h: int, w: int, gs: int, levels_of) -> List[Pass]:
    """The passes of one (h, w) input.  gs = int(max(strides)) (tasks.py:365); levels_of(ph, pw) -> the detection levels of the
    graph at that input size (YoloEngine reads them from its plan's meta["levels"])."""
    sizes = [scaled_size(h, w, r, gs) for r in SCALES]
    wins = clip_windows([levels_of(*padded) for _, padded in sizes])
    return [Pass(r, f, s, p, win) for r, f, (s, p), win in zip(SCALES, FLIPS, sizes, wins)]
