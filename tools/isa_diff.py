"""Compare the gfx950 device code of two builds kernel by kernel: tools/isa_diff.py <objdir_a> <objdir_b>  (needs no GPU).
For every kernel of any object file of A, B must hold exactly one kernel of the same mangled name -- in whichever object file: a
kernel may have moved to another translation unit -- with the same instruction sequence (address / encoding column dropped,
pc-relative literals masked) and the same vgpr / sgpr / agpr counts, LDS size and scratch size (a kernel whose metadata
cannot be read counts as differing).  Prints one line per kernel that differs and a summary line; exits 1 if a kernel differs, is missing, is duplicated or is new in B."""
import re
import sys
from pathlib import Path

from isa_scan import disassemble, kernels, notes

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def instructions(body: str):
    """A kernel's instructions without what depends on where the linker put it."""
    out, getpc = [], -9
    for line in body.splitlines():
        ins = " ".join(line.split("//")[0].split())
        if not ins or ins == "...":  # (objdump's mark for a run of zero bytes: padding between functions)
            continue
        if ins.startswith("s_getpc_b64"):
            getpc = len(out)
        elif len(out) - getpc <= 2 and ins.startswith(("s_add_u32", "s_addc_u32")):  # pc-relative address of a __device__ variable
            ins = re.sub(r"(0x[0-9a-f]+|\d+)$", "<pcrel>", ins)
        out.append(ins)
    while out and out[-1].startswith(("s_nop", "s_code_end")):  # padding up to the next function
        out.pop()
    return out


def load(objdir: Path):
    """{symbol: [(object name, instructions, metadata)]} over every object file of a build directory."""
    ks = {}
    for obj in sorted(objdir.glob("*.o")):
        meta, cur = {}, {}
        for line in notes(obj).splitlines():
            if re.match(r" {0,3}- \.", line):  # an item of the top-level list amdhsa.kernels: a new kernel's record (its arguments' items sit deeper)
                cur = {}
            m = re.match(r"\s*(?:- )?\.(\w+):\s*(\S+)", line)
            if m and m.group(1) in FIELDS:
                cur[m.group(1)] = int(m.group(2))
            elif m and m.group(1) == "symbol":
                meta[m.group(2)[:-3]] = cur  # "<name>.kd"; the record's later keys still land in this dict
        for sym, body in kernels(disassemble(obj)):
            ks.setdefault(sym, []).append((obj.name, instructions(body), meta.get(sym, {})))
    return ks


def main(a: Path, b: Path) -> int:
    ka, kb = load(a), load(b)
    same = bad = 0
    for sym, recs in sorted(ka.items()):
        oa, ia, ma = recs[0]
        if len(recs) != 1 or len(kb.get(sym, ())) != 1:
            print(f"COUNT   {sym}: {len(recs)} in A, {len(kb.get(sym, ()))} in B")
            bad += 1
            continue
        ob, ib, mb = kb[sym][0]
        if set(ma) != set(FIELDS) or set(mb) != set(FIELDS):  # never let a note this parser cannot read pass as "equal"
            print(f"NOMETA  {sym}: figures found {sorted(ma)} in A, {sorted(mb)} in B; expected {list(FIELDS)}")
            bad += 1
            continue
        if ia == ib and ma == mb:
            same += 1
            continue
        bad += 1
        grew = [f for f in FIELDS if mb[f] > ma[f]]
        first = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
        print(f"DIFFER  {sym} ({oa} -> {ob}): {len(ia)} -> {len(ib)} instructions, first difference at {first}; "
              + ", ".join(f"{f} {ma.get(f)} -> {mb.get(f)}" for f in FIELDS if ma.get(f) != mb.get(f))
              + ("; GREW: " + " ".join(grew) if grew else ""))
    new = sorted(set(kb) - set(ka))
    for sym in new:
        print(f"NEW     {sym} ({kb[sym][0][0]})")
    print(f"isa_diff: {len(ka)} kernels in A, {len(kb)} in B: {same} identical, {bad} differ or miscount, {len(new)} only in B")
    return 1 if bad or new else 0


if __name__ == "__main__":
    sys.exit(main(Path(sys.argv[1]), Path(sys.argv[2])))
