"""Case table of the persistent, software-pipelined bf16 GEMM (csrc/gemm_bf16_pp.hpp: tile id 64, UFND_GEMM_TILE_PERSISTENT, K = 768),
built on tests/gemm_bf16_cases.py: the cases are that file's `Case`, made, referenced in float64, checked and emulated by that file's
functions, under that file's bounds.  The kernel's arithmetic is documented as the one-tile kernel's own -- k ascending in steps of 32
per MFMA, the same epilogue expressions -- and tests/test_gpu_gemm_pp.py holds it to that bit for bit, so the derivations of that
docstring apply as they stand; no bound here comes from a GPU result.  Shared by tests/test_gemm_pp_cases.py (CPU: the walk, the
coverage, the plan entry, every refusal, the emulation inside the bounds and eight wrong kernels outside) and
tests/test_gpu_gemm_pp_cases.py (GPU: every case through the C ABI, twice).  NumPy only.

WHAT THE TABLE IS ABOUT.  A workgroup of this form walks a list of 256 x 128 tiles: the epilogue of one tile rides through the K loop of
the next, two accumulator sets alternate, the set left over after an even tile count is copied, every global address is a 32-bit byte
offset built from lda / ldw / ldo / ldrb, and a live-row count may shorten the walk.  `m x n` below means m_tiles x n_tiles, i.e.
M = 256 m, N = 128 n; the tile counts per workgroup are for 256 CUs (walk() restates the kernel's walk; the CPU test recomputes them).
   1 x 8    8 workgroups, 1 tile each: nothing ever rides along an epilogue.  FOLD x {none, GELU, quick-GELU} and PLAIN x {..} in the
            rounded family, the two without an activation in the exact family as well (an activation's argument must stay below
            ACT_RANGE, which the exact family's integers do not)
   2 x 4    the same for RES and RES_LN (out_stats needs N <= 768)
   2 x 5    T = 10 is no multiple of 8; six workgroups with 1 tile, two with 2: the even-count exit (the set copy).  All four modes
   3 x 5    one ragged row group (m_tiles < pp_rows), seven workgroups with 2 tiles
   5 x 3    a full group, then a one-row group
   9 x 1    one column tile per panel
  11 x 24   G = 256 with T = 264 just above it; FOLD + erf-GELU, rounded (the largest shape given a float64 erf)
  25 x 24   2 and 3 tiles per workgroup; the last row group is ragged (25 = 6 x 4 + 1).  FOLD + quick-GELU
  32 x 24   3 tiles everywhere: the geometry the automatic choice picks
  43 x 24   4 and 5 tiles: the second turn of the walk's loop, both exits, a ragged last group (43 = 10 x 4 + 3).  Exact family
 129 x 6    3 and 4 tiles, RES and RES_LN.  Exact family
Across the small shapes (at most 15 tiles): a_parts 2 / 10 / 22 / 24 and r_parts 2 / 12 / 24 (the statistics loader's nq = parts / 2),
no bias in each mode, FOLD with and without the guard pointer and with a NaN statistic, each shape once with tight strides (every
other case has _mk's default strides: all different, all wider than tight).
LIVE ROWS (LiveCase): ufnd_gemm_bf16_live / ufnd_gemm_bf16_ln_live with a device row count, judged against float64 over the live rows:
rows from ceil(live / 256) x 256 on keep their sentinels, the rows between are not judged, statistics rows past `live` hold NaN and
must not reach the guard, and live = 0 writes nothing."""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from tests import gemm_bf16_cases as G
from tests.gemm_bf16_cases import (ACT_GELU, ACT_NONE, ACT_QUICK_GELU, GUARD_SLOTS, MUTANT_FACTOR, PRE, SENT_BF16, SENT_F32,  # noqa: F401
                                   Case, _mk, check, emulate, is_bit_exact, make, reference, unequal)

PP = G.PP_TILE
BM, BN = G.PP_DIMS[:2]
K = 768
PP_ROWS = 4                        # launch_pp: row panels per group of the walk order
A_PARTS = (2, 10, 22, 24)
R_PARTS = (2, 12, 24)
MODES = ("plain", "fold", "rln", "res")      # pp::PLAIN, FOLD, RES_LN, RES, in the enum's order
INSTANTIATIONS = tuple([("fold", a) for a in (0, 1, 2)] + [("plain", a) for a in (0, 1, 2)] + [("rln", 0), ("res", 0)])
SMALL_TILES = 15


def mode_of(c: Case) -> str:
    """pp_mode_of, from the case's fields"""
    if c.ln == "fold":
        return "fold"
    if c.res == "bf16":
        return "rln" if c.ln == "rln" else "res"
    return "plain"


def _pp(mode: str, m: int, n: int, family: str, *, act=0, parts=0, bias=True, guard="no", tight=False, edge="") -> Case:
    kw = dict(tight=tight, bias=bias, outs="bf16", act=act, edge=edge, tag=f"{m}x{n}")
    if mode == "plain":
        return _mk("ex", PP, BM * m, BN * n, K, family, **kw)
    if mode == "fold":
        return _mk("ln", PP, BM * m, BN * n, K, family, ln="fold", parts=parts or 24, guard=guard, **kw)
    if mode == "rln":
        return _mk("ln", PP, BM * m, BN * n, K, family, ln="rln", parts=parts or 24, res="bf16", out_stats=True, **kw)
    return _mk("ln", PP, BM * m, BN * n, K, family, ln="plain", res="bf16", out_stats=True, **kw)


def _cases() -> List[Case]:
    out: List[Case] = []
    # ---- one tile per workgroup: every instantiation
    e = "1 tile per workgroup: no epilogue rides along"
    for i, (mode, act) in enumerate(INSTANTIATIONS):
        m, n = (1, 8) if mode in ("fold", "plain") else (2, 4)
        out.append(_pp(mode, m, n, "rounded", act=act, parts=(A_PARTS if mode == "fold" else R_PARTS)[i % 3], guard="yes" if act == 1 else "no", edge=e))
        if act == ACT_NONE:
            out.append(_pp(mode, m, n, "exact", parts=24 if mode == "fold" else 2, guard="yes", edge=e))
    out.append(_pp("plain", 1, 8, "exact", tight=True, edge=e + "; tight strides"))
    out.append(_pp("rln", 2, 4, "exact", parts=12, tight=True, edge=e + "; tight strides"))
    # ---- 2 x 5: T % 8 != 0, the even-count exit
    e = "T = 10: six workgroups with 1 tile, two with 2 (the set copy)"
    out.append(_pp("plain", 2, 5, "exact", edge=e))
    out.append(_pp("fold", 2, 5, "exact", parts=22, guard="yes", edge=e))
    out.append(_pp("rln", 2, 5, "exact", parts=12, edge=e))
    out.append(_pp("res", 2, 5, "exact", edge=e))
    out.append(_pp("fold", 2, 5, "rounded", act=ACT_GELU, parts=10, edge=e))
    out.append(_pp("plain", 2, 5, "exact", bias=False, edge=e + "; no bias"))
    out.append(_pp("fold", 2, 5, "rounded", parts=2, bias=False, guard="yes", edge=e + "; no bias"))
    out.append(_pp("rln", 2, 5, "exact", parts=24, bias=False, edge=e + "; no bias"))
    out.append(_pp("res", 2, 5, "exact", bias=False, edge=e + "; no bias"))
    out.append(_pp("fold", 2, 5, "rounded", parts=24, guard="nan", tight=True, edge=e + "; a NaN statistic must report +inf; tight strides"))
    # ---- ragged row groups of the walk order
    e = "one ragged row group (3 < pp_rows), seven workgroups with 2 tiles"
    out.append(_pp("plain", 3, 5, "exact", edge=e))
    out.append(_pp("rln", 3, 5, "exact", parts=2, edge=e))
    out.append(_pp("rln", 3, 5, "rounded", parts=24, tight=True, edge=e + "; tight strides"))
    e = "a full row group, then a one-row group"
    out.append(_pp("plain", 5, 3, "exact", edge=e))
    out.append(_pp("rln", 5, 3, "exact", parts=24, edge=e))
    out.append(_pp("plain", 5, 3, "rounded", act=ACT_QUICK_GELU, tight=True, edge=e + "; tight strides"))
    e = "one column tile per panel"
    out.append(_pp("plain", 9, 1, "exact", edge=e))
    out.append(_pp("res", 9, 1, "exact", edge=e))
    out.append(_pp("res", 9, 1, "exact", tight=True, edge=e + "; tight strides"))
    # ---- several tiles per workgroup
    out.append(_pp("fold", 11, 24, "rounded", act=ACT_GELU, parts=24, guard="yes", edge="G = 256, T = 264 just above it"))
    out.append(_pp("fold", 25, 24, "rounded", act=ACT_QUICK_GELU, parts=24, guard="yes", edge="2 and 3 tiles per workgroup, ragged last row group"))
    out.append(_pp("fold", 32, 24, "rounded", act=ACT_QUICK_GELU, parts=24, guard="yes", edge="3 tiles everywhere: what the automatic choice picks"))
    out.append(_pp("fold", 43, 24, "exact", parts=24, guard="yes", edge="4 and 5 tiles: the loop's second turn, both exits, ragged last group"))
    out.append(_pp("plain", 43, 24, "exact", edge="4 and 5 tiles: the loop's second turn, both exits, ragged last group"))
    out.append(_pp("res", 129, 6, "exact", edge="3 and 4 tiles per workgroup on the residual forms"))
    out.append(_pp("rln", 129, 6, "exact", parts=24, edge="3 and 4 tiles per workgroup on the residual forms"))
    return out


CASES: List[Case] = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "case ids collide"
SMALL = [c for c in CASES if (c.M // BM) * (c.N // BN) <= SMALL_TILES]
# PLAIN, tight (the stamps entry of the diagnostics library takes no strides): the tile count every workgroup reports against walk()
STAMP_CASES = [_pp("plain", m, n, "exact", tight=True, edge="stamps: tiles per workgroup") for m, n in ((2, 5), (25, 24), (43, 24))]


class LiveCase(NamedTuple):
    case: Case                     # the launch at its capacity M
    m_live: int                    # the row count on the device (may exceed M: clamped)

    @property
    def id(self) -> str:
        return f"{self.case.id}-live{self.m_live}"

    @property
    def live(self) -> int:
        return min(max(self.m_live, 0), self.case.M)

    @property
    def panel_end(self) -> int:
        return (self.live + BM - 1) // BM * BM


def _live_cases() -> List[LiveCase]:
    out = []
    for c in (_pp("plain", 8, 1, "exact", edge="live rows"), _pp("rln", 5, 6, "exact", parts=12, edge="live rows"),
              _pp("fold", 5, 6, "rounded", parts=10, guard="yes", edge="live rows")):
        for n in (0, 1, 255, 256, 257, c.M - 100, c.M, c.M + 5):
            out.append(LiveCase(c, n))
    return out


LIVE_CASES: List[LiveCase] = _live_cases()


# ---------------------------------------------------------------------------------------------------------------------
# the walk
def xcd_contiguous_id(n: int, total: int) -> int:
    """common.hpp: hardware workgroup id n (dealt round-robin over the eight XCDs) -> a logical id that is contiguous per XCD"""
    q, r, xcd, idx = total >> 3, total & 7, n & 7, n >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def grid(m_tiles: int, n_tiles: int, cus: int) -> int:
    return min(cus, m_tiles * n_tiles) & ~7


def walk(m_tiles: int, n_tiles: int, cus: int, live_rows: Optional[int] = None, mutant: Optional[str] = None) -> List[List[Tuple[int, int]]]:
    """Host mirror of gemm_pp_kernel's tile walk: per blockIdx.x, in order, the (row panel, column tile) pairs the workgroup computes.
    The grid comes from the capacity (m_tiles), the tile order from the live panels."""
    g = grid(m_tiles, n_tiles, cus)
    live_tiles = m_tiles
    if live_rows is not None:
        live_tiles = (min(max(live_rows, 0), m_tiles * BM) + BM - 1) // BM
    T, gpx = live_tiles * n_tiles, g >> 3

    def coords(u):
        per = PP_ROWS * n_tiles
        rg, rem = divmod(u, per)
        rows = min(live_tiles - rg * PP_ROWS, PP_ROWS)
        if mutant == "ragged_row_group_walked_as_full":
            rows = PP_ROWS
        tn = rem // rows
        return rg * PP_ROWS + (rem - tn * rows), tn
    out = []
    for b in range(g):
        L = xcd_contiguous_id(b, g)
        xcd = L // gpx
        u, u_end = ((xcd * T) >> 3) + (L - xcd * gpx), ((xcd + 1) * T) >> 3
        mine = []
        while u < u_end:
            mine.append(coords(u))
            u += gpx
        out.append(mine)
    return out


def walk_of(c: Case, cus: int, live_rows: Optional[int] = None, mutant: Optional[str] = None):
    return walk(c.M // BM, c.N // BN, cus, live_rows, mutant)


def ragged_panels(m_tiles: int) -> range:
    """row panels of a last row group that is not full"""
    return range(m_tiles // PP_ROWS * PP_ROWS, m_tiles)


def coverage_gaps(cases: List[Case], lives: List[LiveCase], cus: int, geometry: Optional[Dict] = None) -> List[str]:
    """what the table does NOT reach on a device of `cus` CUs.  geometry: case id -> (m_tiles, n_tiles) as the library plans them
    (the CPU test passes the plan entry's answers); without it the table's own."""
    def geo(c):
        return geometry[c.id] if geometry is not None else (c.M // BM, c.N // BN)
    gaps = []
    counts, exits, ragged_multi = set(), set(), False
    for c in cases:
        m, n = geo(c)
        for mine in walk(m, n, cus):
            counts.add(len(mine))
            if mine:
                exits.add(len(mine) % 2)
            if len(mine) >= 2 and any(p in ragged_panels(m) for p, _ in mine):
                ragged_multi = True
    for lc in lives:
        m, n = geo(lc.case)
        counts.update(len(mine) for mine in walk(m, n, cus, lc.m_live) if not mine)
    for k in (0, 1, 2, 3, 4, 5):
        if k not in counts:
            gaps.append(f"no workgroup with {k} tiles" + (" (live rows)" if k == 0 else ""))
    for par, name in ((1, "odd tile count: the last tile in the first accumulator set"), (0, "even tile count: the set copy")):
        if par not in exits:
            gaps.append(f"exit of the walk: {name}")
    if not any(k >= 4 and k % 2 == 0 for k in counts) or not any(k >= 5 and k % 2 == 1 for k in counts):
        gaps.append("the loop's second turn with both exits (an even and an odd count above 3)")
    if not ragged_multi:
        gaps.append("a ragged row group owned by a workgroup with at least 2 tiles")
    have = {(mode_of(c), c.act) for c in cases}
    gaps += [f"instantiation {mode} act {act}" for mode, act in INSTANTIATIONS if (mode, act) not in have]
    small = [c for c in cases if geo(c)[0] * geo(c)[1] <= SMALL_TILES]
    gaps += [f"a_parts {p}" for p in A_PARTS if not any(mode_of(c) == "fold" and c.parts == p for c in small)]
    gaps += [f"r_parts {p}" for p in R_PARTS if not any(mode_of(c) == "rln" and c.parts == p for c in small)]
    for mode in MODES:
        if not any(mode_of(c) == mode and not c.bias for c in small):
            gaps.append(f"no bias in mode {mode}")
    for shape in sorted({geo(c) for c in small}):
        at = [c for c in small if geo(c) == shape]
        if not any(c.lda == c.K and c.ldw == c.K and c.ldo == c.N and (c.res != "bf16" or c.ldrb == c.N) for c in at):
            gaps.append(f"tight strides at {shape}")
        if not any(c.lda > c.K and c.ldw > c.K and c.ldo > c.N and len({c.lda, c.ldw, c.ldo, c.ldrb}) == 4 for c in at):
            gaps.append(f"wide, pairwise different strides at {shape}")
    fold = [c for c in small if mode_of(c) == "fold"]
    gaps += [f"fold guard {g}" for g in ("no", "yes", "nan") if not any(c.guard == g for c in fold)]
    for fam in ("exact", "rounded"):
        gaps += [f"family {fam}: {mode}" for mode in MODES if not any(mode_of(c) == mode and c.family == fam for c in cases)]
    return gaps


# ---------------------------------------------------------------------------------------------------------------------
# live rows
def make_live(lc: LiveCase, inp: Dict) -> Dict:
    """make(lc.case)'s buffers with the statistics rows past the live count poisoned (copies; `inp` stays as it is)"""
    out = dict(inp)
    for k in ("a_stats", "r_stats"):
        if k in out:
            out[k] = out[k].copy()
            out[k][lc.live:] = np.nan
    return out


def check_live(lc: LiveCase, inp: Dict, got: Dict, cus: int, refs: Optional[Dict] = None) -> Dict[str, float]:
    """G.check over the live rows.  The rows between `live` and the end of its panel are computed and stored by the kernel and read by
    nobody: not judged.  Everything from the panel's end on must hold its sentinel; guard slots from G (of the capacity) on stay 0."""
    c = lc.case
    if lc.live == 0:
        return {k: (0.0 if np.array_equal(got[k], inp[k]) else math.inf) for k in got}
    cl = c._replace(M=lc.live)
    refs = dict(reference(cl, inp) if refs is None else refs)
    view = {}
    for k, v in got.items():
        v = v.copy()
        if k in ("ob", "ostats"):
            v[PRE + lc.live:PRE + lc.panel_end] = SENT_BF16 if k == "ob" else SENT_F32
        view[k] = v
    guard = refs.pop("guard", None)
    out = check(cl, inp, view, refs, cus)
    if guard is not None:
        g = got["guard"]
        r = G.worst_ratio(np.array(float(g.max()) if not np.isnan(g).any() else np.nan), guard[0], guard[1])
        if (g[min(G.planned_grid(c, cus), GUARD_SLOTS):] != 0).any() or (g < 0).any():
            r = math.inf
        out["guard"] = r
    return out


def live_refs(lc: LiveCase, inp: Dict) -> Optional[Dict]:
    return reference(lc.case._replace(M=lc.live), inp) if lc.live else None


def unequal_live(lc: LiveCase, got: Dict, refs: Optional[Dict]) -> int:
    return unequal(lc.case._replace(M=lc.live), got, refs) if lc.live else 0


# ---------------------------------------------------------------------------------------------------------------------
# the emulation of a launch as this form stores it (tile by tile, along the walk) and eight wrong kernels
MUTANTS = ("second_tile_stored_at_first_tiles_coordinates", "statistics_of_the_next_tile_in_the_epilogue", "partial_beyond_count_not_zeroed",
           "ragged_row_group_walked_as_full", "residual_rows_read_with_ldo", "out_stats_rows_strided_by_the_tiles_partials",
           "missing_bias_read_as_present", "dead_rows_of_the_live_panel_enter_the_guard")


def _tile(buf: np.ndarray, p: int, t: int, per_tile_cols: int):
    return buf[PRE + p * BM:PRE + (p + 1) * BM, t * per_tile_cols:(t + 1) * per_tile_cols]


def emulate_pp(c: Case, inp: Dict, order: int = 0, mutant: Optional[str] = None, cus: int = G.PP_CUS, live_rows: Optional[int] = None) -> Dict:
    """G.emulate's float32 restatement of the arithmetic, stored tile by tile along walk(): what no workgroup computes keeps its
    sentinel.  With live_rows the statistics rows past the count are expected to be poisoned (make_live)."""
    src = inp
    cc = c
    if mutant == "residual_rows_read_with_ldo":
        src = dict(inp)
        flat = G._flat_load(inp["resb"], 0, c.ldrb, c.ldo, c.M, c.N)
        src["resb"] = inp["resb"].copy()
        src["resb"][:c.M, :c.N] = flat
    if mutant == "missing_bias_read_as_present":      # (the absent vector's load reads the first four bytes of W and is to be ignored)
        assert not c.bias
        cc = c._replace(bias=True)
        src = dict(inp)
        src["bias"] = np.full(c.N + G.VEC_PAD, np.ascontiguousarray(inp["W"][0, :2]).view(np.float32)[0], np.float32)
    full = emulate(cc, src, order, mutant if mutant == "partial_beyond_count_not_zeroed" else None)
    tiles = walk_of(c, cus, live_rows, mutant if mutant == "ragged_row_group_walked_as_full" else None)
    m_tiles, n_tiles = c.M // BM, c.N // BN
    alt = {}
    if mutant == "statistics_of_the_next_tile_in_the_epilogue":
        key = "a_stats" if "a_stats" in inp else "r_stats"
        for d in {(mine[i + 1][0] - mine[i][0]) % m_tiles for mine in tiles for i in range(len(mine) - 1)} - {0}:
            s = dict(inp)
            s[key] = inp[key].copy()
            s[key][:c.M] = np.roll(inp[key][:c.M], -d * BM, axis=0)
            alt[d] = emulate(c, s, order)
    got = {k: inp[k].copy() for k in ("ob", "ostats") if k in inp}
    gp = c.N // 32 * 2 // n_tiles                      # floats of a statistics row that one column tile writes
    if "guard" in inp:
        got["guard"] = inp["guard"].copy()
        mean, rstd = G._stats32(inp["a_stats"][:c.M], c.K, G.EPS, mutant)
        with np.errstate(invalid="ignore"):
            ratio = np.abs(mean) * rstd
        ratio = np.where(np.isnan(ratio), np.float32(np.inf), ratio)
        if live_rows is not None and mutant != "dead_rows_of_the_live_panel_enter_the_guard":
            ratio[min(max(live_rows, 0), c.M):] = 0.0
    for b, mine in enumerate(tiles):
        for i, (p, t) in enumerate(mine):
            if p >= m_tiles:
                continue                               # (a walk past the last panel: its stores land behind the capacity)
            sp, st_ = (mine[0] if mutant == "second_tile_stored_at_first_tiles_coordinates" and i == 1 else (p, t))
            data = full
            if alt and i + 1 < len(mine) and (mine[i + 1][0] - p) % m_tiles:
                data = alt[(mine[i + 1][0] - p) % m_tiles]
            _tile(got["ob"], sp, st_, BN)[:] = _tile(data["ob"], p, t, BN)
            if "ostats" in got:
                if mutant == "out_stats_rows_strided_by_the_tiles_partials":
                    flat = got["ostats"].ravel()
                    rows = np.arange(p * BM, (p + 1) * BM)[:, None]
                    idx = PRE * got["ostats"].shape[1] + (rows * 4 + t * 4) * 2 + np.arange(gp)[None, :]
                    flat[idx] = _tile(data["ostats"], p, t, gp)
                else:
                    _tile(got["ostats"], sp, st_, gp)[:] = _tile(data["ostats"], p, t, gp)
            if "guard" in got:
                got["guard"][b % GUARD_SLOTS] = max(got["guard"][b % GUARD_SLOTS], ratio[p * BM:(p + 1) * BM].max())
    return got
