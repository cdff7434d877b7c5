"""Rows with hand-derived answers, an independent brute-force statement of the start-state rule and random batches for the curriculum
tests (host and GPU).  The fields are those of tests/shaping_cases.py: map 0 is the corridor SERPENT_5X4 (the hop count between two free
cells is the difference of their places along it), map 1 SPLIT_3X3 (columns x = 0 and x = 2 do not reach each other).

The free cells of map 0 in cell-index order (k = ix * 4 + iy) and their places along the corridor:

    rank   0  1  2  3  4  5  6  7  8  9 10 11 12 13
    cell   0  1  2  3  7  8  9 10 11 12 16 17 18 19
    place  0  1  2  3  4  8  7  6  5  9 10 11 12 13

The draws.  ``U_TOP = 0x3F7FFFFF`` is the largest u below 1: u (*) float(cnt) stays below cnt for every cnt (the exact product cnt - cnt
2^-24 lies at least half an ulp below cnt), so it truncates to cnt - 1 -- the ``min`` in the rule is reached only by u = 1.0, which lies
outside [0, 1) and is here as ``U_ONE`` to pin the clamp.  ``U_UP_9_OF_14 = 0x3F249249`` is a u whose EXACT product with 14 lies below 9
while the rounded fp32 product is 9.0: rank 9, where exact arithmetic would say 8."""
from fractions import Fraction

import numpy as np

from tests.navigation_cases import NONE, centre
from tests.shaping_cases import CORRIDOR, SERPENT_5X4, SPLIT_3X3, make_field  # noqa: F401  (re-exported)

u32 = lambda bits: float(np.uint32(bits).view(np.float32))
U_TOP, U_ONE, U_UP_9_OF_14 = u32(0x3F7FFFFF), 1.0, u32(0x3F249249)
assert Fraction(U_UP_9_OF_14) * 14 < 9 and float(np.float32(U_UP_9_OF_14) * np.float32(14)) == 9.0
OFF = (-1, -1)
P = lambda s: centre(*CORRIDOR[s])            # the centre of the corridor's place s
X = None                                       # "not written"


def rows_2v1():
    """A = 3: cop_0, cop_1, thief_0 (n_cops = 2).  Placement order thief_0, cop_0, cop_1 reads u[0], u[1], u[2].  ``pos``: the expected
    positions in ENV order (cop_0, cop_1, thief_0), or X where the row must stay unwritten (``placed`` 0)."""
    return [
        # thief rank 0 = place 0; the places 2 .. 3 hops away in cell order: 2, 3 -> cop_0 rank 0 = place 2; cop_1: only 3 is left
        dict(name="zeros", map=0, mask=1, band=(2, 3), u=(0.0, 0.0, 0.0), pos=[P(2), P(3), P(0)]),
        # thief int(14 u) = 13 = place 13; 2 .. 3 hops away in cell order: places 10, 11 -> cop_0 int(2 u) = 1 = place 11; cop_1: place 10
        dict(name="top", map=0, mask=1, band=(2, 3), u=(U_TOP, U_TOP, U_TOP), pos=[P(11), P(10), P(13)]),
        # thief: the product rounds up to 9.0: rank 9 = place 9 = cell (3, 0); 1 .. 2 hops away in cell order: places 8, 7, 10, 11;
        # cop_0 int(4 * .5) = 2 -> place 10; cop_1 among 8, 7, 11: int(3 u) = 2 -> place 11
        dict(name="rounds up", map=0, mask=1, band=(1, 2), u=(U_UP_9_OF_14, 0.5, U_TOP), pos=[P(10), P(11), P(9)]),
        # u = 1.0 (outside [0, 1)): min(13, 14) = 13 = place 13; 13 hops away: place 0 alone -> cop_0; cop_1 finds nothing: fallback
        dict(name="u = 1, then nothing left", map=0, mask=1, band=(13, 13), u=(U_ONE, 0.0, 0.0), pos=X),
        dict(name="u = 1, one cop's worth", map=0, mask=1, band=(12, 13), u=(U_ONE, U_ONE, U_ONE), pos=[P(1), P(0), P(13)]),
        dict(name="empty band", map=0, mask=1, band=(14, 20), u=(0.0, 0.0, 0.0), pos=X),
        dict(name="off", map=0, mask=1, band=OFF, u=(0.0, 0.0, 0.0), pos=X),
        dict(name="lo < 1", map=0, mask=1, band=(0, 3), u=(0.0, 0.0, 0.0), pos=X),
        dict(name="lo > hi", map=0, mask=1, band=(3, 2), u=(0.0, 0.0, 0.0), pos=X),
        dict(name="hi = NONE", map=0, mask=1, band=(1, 65535), u=(0.0, 0.0, 0.0), pos=X),
        dict(name="hi = 65534", map=0, mask=1, band=(13, 65534), u=(0.0, 0.0, 0.0), pos=X),        # a valid band: place 13, then nothing
        dict(name="not masked", map=0, mask=0, band=(2, 3), u=(0.0, 0.0, 0.0), pos=X),
        # map 1: thief (0, 0); 1 hop: (0, 1), 2 hops: (0, 2); nothing across the wall
        dict(name="split", map=1, mask=1, band=(1, 2), u=(0.0, 0.0, 0.0), pos=[centre(0, 1), centre(0, 2), centre(0, 0)]),
        dict(name="split, one candidate", map=1, mask=1, band=(1, 1), u=(0.0, 0.0, 0.0), pos=X),
        # thief int(6 * .5) = 3 = cell 6 = (2, 0): the other column
        dict(name="split, right column", map=1, mask=1, band=(1, 2), u=(0.5, U_TOP, 0.0), pos=[centre(2, 2), centre(2, 1), centre(2, 0)]),
    ]


def rows_1v2():
    """A = 3: cop_0, thief_0, thief_1 (n_cops = 1).  Placement order thief_0 (anchor), thief_1, cop_0."""
    return [
        # anchor cell 6 = (2, 0); thief_1 among the cells the anchor reaches, not taken: (2, 1), (2, 2): int(2 u) = 1 -> (2, 2); the cop 1 hop
        # from the nearer thief and not taken: (2, 1)
        dict(name="split", map=1, mask=1, band=(1, 1), u=(0.5, U_TOP, 0.0), pos=[centre(2, 1), centre(2, 0), centre(2, 2)]),
        # anchor place 0, thief_1 rank int(13 * .5) = 6 of the 13 others (cell order: places 1 2 3 4 8 7 6 ...) = place 6;
        # 3 hops from the nearer thief: places 3 (from 0: 3, from 6: 3) and 9 (from 6); cell order 3, 9 -> int(2 u) = 1 -> place 9
        dict(name="corridor", map=0, mask=1, band=(3, 3), u=(0.0, 0.5, U_TOP), pos=[P(9), P(0), P(6)]),
    ]


def batch(rows, A):
    """The rows as arrays: mask uint8 [N], uniform float32 [A, N], band int32 [N, 2], slot_map int32 [N], placed uint8 [N] and positions
    float64 [N, A, 2] (NaN where the row must stay unwritten)."""
    N = len(rows)
    pos = np.full((N, A, 2), np.nan)
    for n, r in enumerate(rows):
        if r["pos"] is not X:
            pos[n] = np.array(r["pos"], np.float64)
    return dict(mask=np.array([r["mask"] for r in rows], np.uint8), uniform=np.array([r["u"] for r in rows], np.float32).T.copy(),
                band=np.array([r["band"] for r in rows], np.int32), slot_map=np.array([r["map"] for r in rows], np.int32),
                placed=np.array([r["pos"] is not X for r in rows], np.uint8), positions=pos)


def random_batch(seed, N, A, n_maps=2, hi_max=6):
    """Random rows: mixed masks, bands (valid, off, lo < 1, lo > hi, empty) and draws with the special u values in them."""
    rng = np.random.default_rng(seed)
    mask = (rng.random(N) < 0.7).astype(np.uint8)
    lo = rng.integers(1, hi_max + 1, N)
    band = np.stack([lo, lo + rng.integers(0, 4, N)], axis=1).astype(np.int32)
    kind = rng.random(N)
    band[kind < 0.10] = OFF
    band[(kind >= 0.10) & (kind < 0.15)] = (0, 3)
    band[(kind >= 0.15) & (kind < 0.20)] = (4, 2)
    band[(kind >= 0.20) & (kind < 0.25)] = (40, 50)          # valid and empty on these fields
    u = rng.random((A, N), dtype=np.float32)
    special = np.array([0.0, U_TOP, U_UP_9_OF_14, 0.5, u32(0x3F6DB6DB), u32(0x3F555555)], np.float32)
    pick = rng.random((A, N)) < 0.25
    u[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return mask, u, band, rng.integers(0, n_maps, N).astype(np.int32)


def brute_force(mask, uniform, band, tables, slot_map, n_cops, cell=16):
    """The rule, slot by slot and cell by cell, from its statement alone: ``tables[m] = (free uint8 [C], hops uint16 [C, C], Hc)``.  Returns
    (cells int64 [N, A] in ENV order, -1 where nothing was placed; placed uint8 [N])."""
    A, N = uniform.shape
    nt = A - n_cops
    cells, placed = np.full((N, A), -1, np.int64), np.zeros(N, np.uint8)
    for n in range(N):
        lo, hi = int(band[n, 0]), int(band[n, 1])
        if not mask[n] or not 1 <= lo <= hi <= 65534:
            continue
        free, hops, _ = tables[int(slot_map[n])]
        chosen = []
        for i in range(A):
            cand = []
            for k in np.flatnonzero(free):
                if k in chosen:
                    continue
                if i == 0:
                    ok = True
                elif i < nt:
                    ok = hops[chosen[0], k] != NONE
                else:
                    d = [int(hops[b, k]) for b in chosen[:nt] if hops[b, k] != NONE]
                    ok = bool(d) and lo <= min(d) <= hi
                if ok:
                    cand.append(int(k))
            if not cand:
                break
            j = min(len(cand) - 1, int(np.float32(uniform[i, n]) * np.float32(len(cand))))
            chosen.append(cand[j])
        else:
            placed[n] = 1
            cells[n, n_cops:] = chosen[:nt]
            cells[n, :n_cops] = chosen[nt:]
    return cells, placed


def centres(cells, tables, slot_map, cell=16):
    """float64 [N, A, 2]: the centres of ``cells`` (NaN where -1)."""
    Hc = np.array([tables[int(m)][2] for m in slot_map], np.int64).reshape(-1, 1)
    out = np.stack([(cells // Hc + 0.5) * cell, (cells % Hc + 0.5) * cell], axis=2).astype(np.float64)
    out[cells < 0] = np.nan
    return out


def tables_of(field):
    return [(field.free_of(m), field.hops_of(m), int(field.grid_host[m, 1])) for m in range(field.n_maps)]
