"""Per-segment episode summaries, host side: include/cat_episodes.h <-> libcat_learn.so <-> the ctypes mirror, and
``EpisodeTracker.segment_summary`` on CPU tensors -- per segment the ``summary()`` of a tracker that was fed that segment's slots alone,
integers equal and doubles bit-equal."""
import ctypes as C
import re
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

from as_cops_and_thieves_amd import _learn_native as ln
from as_cops_and_thieves_amd.episodes import EpisodeTracker, halving_tree_sum

ROOT = Path(__file__).resolve().parents[1]
AGENTS = ["cop_0", "cop_1", "thief_0"]


def bits(x) -> bytes:
    return struct.pack("<d", x)


def test_header_library_and_mirror_agree():
    ln.build()
    L = ln.lib()
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_episodes.h").read_text(), flags=re.S)
    assert int(re.search(r"#define CAT_EPISODES_MAX_SEGMENTS (\d+)", code).group(1)) == ln.EPISODES_MAX_SEGMENTS == ln.ACT_MAX_SEGMENTS == 32
    assert int(re.search(r"#define CAT_EPISODES_ABI_VERSION (\d+)", code).group(1)) == 1 == L.cat_episodes_abi_version()
    m = re.search(r"int\s+\(?\s*cat_episodes_segment_summary\s*\)?\s*\(([^)]*)\)\s*;", code)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["const cat_episodes_segment_summary_args *a", "void *stream"]
    assert ln.EPISODE_SEGMENTS_SYMBOLS == ("cat_episodes_segment_summary",) and hasattr(L, "cat_episodes_segment_summary")
    body = re.search(r"typedef struct cat_episodes_segment_summary_args \{(.*?)\} cat_episodes_segment_summary_args;", code, re.S).group(1)
    body = re.sub(r"\[[^\]]*\]", "", body)
    names = [n for decl in body.split(";") for n in re.findall(r"\b([A-Za-z_0-9]+)\s*(?=,|$)", decl.strip())]
    assert names == [f[0] for f in ln.EpisodesSegmentSummary._fields_]
    # three int32, 33 bounds (144 bytes: the pointers that follow are 8-aligned without padding), quota, the state, out
    assert C.sizeof(ln.EpisodesSegmentSummary) == 3 * 4 + 33 * 4 + 8 + C.sizeof(ln.EpisodesState) + 8 == 256
    assert ln.EpisodesSegmentSummary.quota.offset == 144 and ln.EpisodesSegmentSummary.out.offset == 248


def test_entry_refuses_bad_arguments_before_touching_a_device():
    L = ln.lib()
    fn = L.cat_episodes_segment_summary
    err = L.cat_episodes_last_error

    def args(N, A, S, start):
        return ln.EpisodesSegmentSummary(N, A, S, (C.c_int32 * 33)(*start))
    assert fn(None, None) == -1 and b"dimensions" in err()
    for N, A in ((0, 2), (8, 0), (8, 9)):
        assert fn(C.byref(args(N, A, 1, [0, N])), None) == -1 and b"dimensions" in err(), (N, A)
    for S, start in ((0, [0]), (33, list(range(33))), (-1, [0, 8]), (2, [1, 4, 8]), (2, [0, 4, 7]), (2, [0, 4, 9]), (3, [0, 4, 4, 8]), (3, [0, 5, 4, 8])):
        assert fn(C.byref(args(8, 2, S, start)), None) == -1 and b"segments" in err(), (S, start)
    assert fn(C.byref(args(8, 2, 2, [0, 4, 8])), None) == -1 and b"NULL" in err()           # the table is fine, every buffer is NULL


BAD_BOUNDS = [[], [0], [0, 5], [1, 12], [0, 4, 4, 12], [0, 7, 5, 12], [0, 13], [0, 4.5, 12], list(range(33)) + [40], None, "0,12", [0, -3, 12]]


@pytest.mark.parametrize("bad", BAD_BOUNDS, ids=[str(b) for b in BAD_BOUNDS])
def test_bad_bounds_raise_value_error_in_both_layers(bad, monkeypatch):
    monkeypatch.setattr(ln, "lib", lambda: pytest.fail("the library was touched"))
    n = 40 if bad is not None and len(bad) == 34 else 12
    tr = EpisodeTracker(n, AGENTS, 10)
    with pytest.raises(ValueError):
        tr.segment_summary(bad)
    with pytest.raises(ValueError):
        ln.episodes_segment_summary(tr.state, None, bad, torch.zeros(32 * C.sizeof(ln.EpisodesSummaryBlock), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ln.segment_bounds(n, bad)


def _streams(T, N, A, rng):
    """Random tick streams with rewards spread over many decades, so that the order of the f64 additions shows in the bits."""
    reward = (rng.standard_normal((T, N, A)) * 10.0 ** rng.integers(-4, 5, (T, N, A))).astype(np.float32)
    term = rng.random((T, N)) < 0.2
    trunc = term & (rng.random((T, N)) < 0.3)
    win = np.where(term, np.where(trunc, -1, rng.integers(0, 2, (T, N))), -1).astype(np.int8)
    return tuple(torch.from_numpy(x) for x in (reward, term, trunc, win))


@pytest.mark.parametrize("quota", [None, 2])
def test_each_segment_equals_a_tracker_fed_that_segment_alone(quota):
    rng = np.random.default_rng(5)
    N, T, bounds = 37, 60, [0, 1, 6, 22, 23, 37]                       # lengths 1, 5, 16 (a power of two), 1, 14
    reward, term, trunc, win = _streams(T, N, len(AGENTS), rng)
    whole = EpisodeTracker(N, AGENTS, 30)
    whole.set_quota(quota)
    whole.update(reward, term, trunc, win)
    got = whole.segment_summary(bounds)
    blocks = whole.segment_blocks(bounds)
    assert len(got) == len(blocks) == 5 and sum(g["episodes"] for g in got) == whole.summary()["episodes"] > 50
    differs = False
    for (lo, hi), g, b in zip(zip(bounds[:-1], bounds[1:]), got, blocks):
        part = EpisodeTracker(hi - lo, AGENTS, 30)
        part.set_quota(quota)
        part.update(reward[:, lo:hi], term[:, lo:hi], trunc[:, lo:hi], win[:, lo:hi])
        want = part.summary()
        want.pop("length_hist")
        assert set(g) == set(want) and "length_hist" not in g
        for k, v in want.items():
            assert type(g[k]) is type(v), k
            assert (bits(g[k]) == bits(v)) if isinstance(v, float) else g[k] == v, (lo, hi, k, g[k], v)
        raw = part.summary_block()
        for k in ("ret_sum", "ret_sq"):
            assert [bits(x) for x in b[k]] == [bits(x) for x in raw[k]]
            col = whole.state[k].numpy()[lo:hi]
            assert [bits(x) for x in b[k]] == [bits(float(x)) for x in halving_tree_sum(col)]
            differs |= any(bits(float(x)) != bits(float(y)) for x, y in zip(halving_tree_sum(col), np.add.accumulate(col, axis=0)[-1]))
    assert differs, "the data does not tell the halving tree from a left-to-right sum"


def test_one_segment_equals_summary():
    rng = np.random.default_rng(9)
    tr = EpisodeTracker(13, AGENTS, 30)
    tr.update(*_streams(40, 13, len(AGENTS), rng))
    want = tr.summary()
    want.pop("length_hist")
    (got,) = tr.segment_summary([0, 13])
    assert list(got) == list(want)
    assert all((bits(got[k]) == bits(v)) if isinstance(v, float) else got[k] == v for k, v in want.items())


def test_default_episode_stats_signature_is_unchanged():
    import inspect
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    p = inspect.signature(VecCopsEnv.episode_stats).parameters
    assert list(p) == ["self", "clear", "segments"] and p["clear"].default is False and p["segments"].default is None
