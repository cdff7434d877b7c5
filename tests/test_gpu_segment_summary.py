"""``cat_episodes_segment_summary`` on the GPU (include/cat_episodes.h): every segment's block bit-equal to ``cat_episodes_summary`` launched
on the sliced state and to ``halving_tree_sum`` on the host, guard blocks untouched, capturable, bad arguments refused before a device call."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# A: lengths on and either side of the 1024-thread block, a power of two, leaf folds with K = 2 and K = 4 and a ragged tail.  B: 32 tiny segments.
CASES = {"A": (3, [1, 1023, 1024, 1025, 2049, 3000]), "B": (1, [3] * 32)}
INT_FIELDS = ("episodes", "cop_wins", "thief_wins", "timeouts", "open_slots", "len_sum", "len_min", "len_max")


def _bounds(lengths):
    return [0] + [int(v) for v in np.cumsum(lengths)]


@functools.lru_cache(maxsize=None)
def _filled(case):
    """A device tracker whose per-slot state is random: f64 sums of mixed sign over about nine decades, so the order of additions shows."""
    import torch
    from as_cops_and_thieves_amd.episodes import EpisodeTracker
    A, lengths = CASES[case]
    N = sum(lengths)
    rng = np.random.default_rng(11 + len(lengths))
    tr = EpisodeTracker(N, [f"a_{i}" for i in range(A)], 200, device="cuda:0")
    host = {"ret_sum": rng.standard_normal((N, A)) * 10.0 ** rng.uniform(-4, 5, (N, A)),
            "ret_sq": rng.standard_normal((N, A)) * 10.0 ** rng.uniform(-4, 5, (N, A)),
            "finished": rng.integers(0, 6, N).astype(np.int32), "cop_wins": rng.integers(0, 4, N).astype(np.int32),
            "thief_wins": rng.integers(0, 4, N).astype(np.int32), "timeouts": rng.integers(0, 3, N).astype(np.int32),
            "len_sum": rng.integers(0, 2 ** 40, N).astype(np.int64), "len_min": rng.integers(1, 200, N).astype(np.int32),
            "len_max": rng.integers(1, 200, N).astype(np.int32)}
    for k, v in host.items():
        tr.state[k].copy_(torch.from_numpy(v))
    quota = rng.integers(0, 6, N).astype(np.int32)
    return tr, host, quota


def _block(raw: bytes, A: int):
    from as_cops_and_thieves_amd import _learn_native as ln
    blk = ln.EpisodesSummaryBlock.from_buffer_copy(raw)
    out = {k: int(getattr(blk, k)) for k in INT_FIELDS}
    out["ret_sum"], out["ret_sq"] = np.array(blk.ret_sum[:]).tobytes(), np.array(blk.ret_sq[:]).tobytes()
    return out


def _assert_the_order_of_additions_shows(case):
    """Host only: a plain left-to-right sum of at least one segment differs in bits from its halving-tree sum -- else the data proves nothing."""
    from as_cops_and_thieves_amd.episodes import halving_tree_sum
    _, host, _ = _filled(case)
    b = _bounds(CASES[case][1])
    assert any(halving_tree_sum(host[k][lo:hi]).tobytes() != np.add.accumulate(host[k][lo:hi], axis=0)[-1].tobytes()
               for lo, hi in zip(b[:-1], b[1:]) for k in ("ret_sum", "ret_sq")), case


@pytest.mark.parametrize("limited", [False, True], ids=["no-quota", "quota"])
@pytest.mark.parametrize("case", list(CASES))
def test_every_segment_equals_the_summary_of_the_sliced_state_and_the_host_tree(case, limited):
    import torch
    from as_cops_and_thieves_amd import _learn_native as ln
    from as_cops_and_thieves_amd.episodes import halving_tree_sum
    _assert_the_order_of_additions_shows(case)
    tr, host, quota_h = _filled(case)
    A, lengths = CASES[case]
    b, S = _bounds(lengths), len(lengths)
    BLOCK = C.sizeof(ln.EpisodesSummaryBlock)
    quota = torch.from_numpy(quota_h).cuda() if limited else None
    guarded = torch.full(((S + 2) * BLOCK,), 0xA5, dtype=torch.uint8, device="cuda:0")         # a guard block on either side
    out = guarded[BLOCK:(S + 1) * BLOCK]
    ln.episodes_segment_summary(tr.state, quota, b, out)
    torch.cuda.synchronize()
    raw = guarded.cpu().numpy().tobytes()
    assert raw[:BLOCK] == b"\xa5" * BLOCK and raw[(S + 1) * BLOCK:] == b"\xa5" * BLOCK
    got = [_block(raw[(1 + s) * BLOCK:(2 + s) * BLOCK], A) for s in range(S)]
    one = torch.zeros(BLOCK, dtype=torch.uint8, device="cuda:0")
    for s, (lo, hi) in enumerate(zip(b[:-1], b[1:])):
        sliced = {k: (v if k == "len_hist" else v[lo:hi]) for k, v in tr.state.items()}         # every per-slot pointer advanced by lo rows
        assert all(v.is_contiguous() for v in sliced.values())
        ln.episodes_summary(sliced, None if quota is None else quota[lo:hi], one)
        want = _block(one.cpu().numpy().tobytes(), A)
        assert got[s] == want, (case, s, lo, hi)
        pad = np.zeros((hi - lo, 8 - A))
        for k in ("ret_sum", "ret_sq"):
            assert got[s][k] == halving_tree_sum(np.concatenate([host[k][lo:hi], pad], axis=1)).tobytes(), (case, s, k)
        assert got[s]["episodes"] == int(host["finished"][lo:hi].sum()) and got[s]["len_sum"] == int(host["len_sum"][lo:hi].sum())
        assert got[s]["len_min"] == int(host["len_min"][lo:hi].min()) and got[s]["len_max"] == int(host["len_max"][lo:hi].max())
        assert got[s]["open_slots"] == (int((host["finished"][lo:hi] < quota_h[lo:hi]).sum()) if limited else 0)
    # the tracker's own reading: the same blocks as Python numbers
    tr.set_quota(quota)
    blocks = tr.segment_blocks(b)
    tr.set_quota(None)
    assert [np.array(x["ret_sum"] + [0.0] * (8 - A)).tobytes() for x in blocks] == [g["ret_sum"] for g in got]
    assert [[x[k] for k in INT_FIELDS] for x in blocks] == [[g[k] for k in INT_FIELDS] for g in got]


def test_the_launch_is_capturable_and_replays_equal_the_eager_result():
    import torch
    from as_cops_and_thieves_amd import _learn_native as ln
    tr, _, quota_h = _filled("A")
    b = _bounds(CASES["A"][1])
    S, BLOCK = len(b) - 1, C.sizeof(ln.EpisodesSummaryBlock)
    quota = torch.from_numpy(quota_h).cuda()
    eager = torch.zeros(S * BLOCK, dtype=torch.uint8, device="cuda:0")
    ln.episodes_segment_summary(tr.state, quota, b, eager)
    out = torch.zeros(S * BLOCK, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ln.episodes_segment_summary(tr.state, quota, b, out)
    for _ in range(2):
        out.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_rejected_arguments_return_bad_arg_without_a_device_call():
    import torch
    from as_cops_and_thieves_amd import _learn_native as ln
    tr, _, _ = _filled("B")
    L = ln.lib()
    N, BLOCK = tr.N, C.sizeof(ln.EpisodesSummaryBlock)
    out = torch.full((33 * BLOCK,), 0x77, dtype=torch.uint8, device="cuda:0")
    state = ln._episodes_state(tr.state)

    def call(n, a, s, start, st=state, o=None):
        args = ln.EpisodesSegmentSummary(n, a, s, (C.c_int32 * 33)(*start), None, st, out.data_ptr() if o is None else o)
        return L.cat_episodes_segment_summary(C.byref(args), ln._stream())
    good = list(range(0, N + 1, 3))
    bad = [(N, 1, 0, [0]), (N, 1, 33, good), (N, 1, 2, [0, 3]), (N, 1, 2, [1, 3, N]), (N, 1, 3, [0, 6, 6, N]), (N, 1, 3, [0, 9, 6, N]),
           (N, 0, 32, good), (N, 9, 32, good), (0, 1, 1, [0, 0])]
    for n, a, s, start in bad:
        assert call(n, a, s, start) == -1 and L.cat_episodes_last_error(), (n, a, s, start)          # CAT_EPISODES_ERR_BAD_ARG
    assert call(N, 1, 32, good, o=0) == -1 and b"NULL" in L.cat_episodes_last_error()
    assert call(N, 1, 32, good, st=ln.EpisodesState()) == -1 and b"NULL" in L.cat_episodes_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0x77).all())                                                                 # nothing was launched
    assert call(N, 1, 32, good) == 0
    torch.cuda.synchronize()
    assert bool((out[:32 * BLOCK] != 0x77).any()) and bool((out[32 * BLOCK:] == 0x77).all())
