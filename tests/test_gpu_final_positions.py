"""GPU: end-of-episode positions (``cat_bind_final_positions``, include/cat_sim.h) -- where an episode ended, which under auto-reset
``team_positions`` no longer shows -- against the two-launch path (``cat_step``, then ``cat_reset_done``) bit for bit, through every stepping
entry, and the capture / timeout maps built on them (``cat_render_positions_ends_update``) against the NumPy form.

Every case has 64 slots, ``max_step_count = 6`` (time-outs) and start positions from ``tests.writeback_cases._place``: the thief of every
fifth slot stands 15 px from cop 0 in an open line, inside the termination radius (captures on the first tick).  A case asserts that both
outcomes occurred -- a condition on its inputs -- and reads the device error word once, at its end."""
import functools

import numpy as np
import pytest

from tests.util import OUT_KEYS, assert_outputs_equal, assert_state_equal, to_np

pytestmark = pytest.mark.gpu

N, MAX_STEP, SENTINEL = 64, 6, 0x7E00
# name -> map, cops, thieves, rays, bbtree_gate, CAT_POOL (None: what cat_create picks), the one-tick kernel it must then run (None: either)
CASES = {
    "squarinth 1v1 r90": ("squarinth", 1, 1, 90, 1, None, None),
    "labyrinth 2v1 r64 pooled": ("labyrinth", 2, 1, 64, 1, "1", "step_kernel_pooled"),
    "labyrinth 2v1 r64 units": ("labyrinth", 2, 1, 64, 1, "0", "step_kernel"),
    "agh-map 2v1 r64 (chunk form)": ("agh-map", 2, 1, 64, 1, None, None),
    "grandbyrinth 3v2 r64": ("grandbyrinth", 3, 2, 64, 1, None, None),
    "lbirinth 2v1 r64 chipmunk order": ("lbirinth", 2, 1, 64, 2, None, None),
}
LAB = "labyrinth 2v1 r64 pooled"


@functools.lru_cache(maxsize=None)
def _case(name):
    """cfg, compiled map, start positions [N, A, 2] and an action tape [24, N, A]: made once per process, never changed."""
    from as_cops_and_thieves_amd.config import SimConfig
    from as_cops_and_thieves_amd.maps import load_preset
    from oracle.cat_oracle import OracleSim
    from tests.writeback_cases import _place
    m, cops, thieves, rays, gate, _, _ = CASES[name]
    cmap = load_preset(m, cops, thieves).compile()
    cfg = SimConfig(n_envs=N, n_cops=cops, n_thieves=thieves, n_rays=rays, max_step_count=MAX_STEP, seed=29, bbtree_gate=gate)
    rng = np.random.default_rng(sorted(CASES).index(name))
    start = _place(OracleSim(cfg, [cmap]), cmap, rng, cops)
    return cfg, cmap, start, rng.integers(0, 4, size=(24, N, cops + thieves), dtype=np.int32)


def _sims(name, monkeypatch, count):
    import torch
    from as_cops_and_thieves_amd.sim import CatSim
    cfg, cmap, start, tape = _case(name)
    pool, kernel = CASES[name][5:]
    if pool is not None:
        monkeypatch.setenv("CAT_POOL", pool)
    sims = [CatSim(cfg, [cmap], device="cuda:0") for _ in range(count)]
    for s in sims:
        if kernel is not None:      # through cat_one_tick_kernel: the pooled and the unit-form kernels are both among the cases
            assert s.one_tick_kernel == kernel and (s.rollout_kernel == "rollout_kernel_pooled") == (kernel == "step_kernel_pooled")
        s.reset(positions=torch.from_numpy(start))
    return sims, torch.from_numpy(tape).to("cuda:0")


def _sentinel(*shape):
    import torch
    return torch.full(shape, SENTINEL, dtype=torch.int16, device="cuda:0").view(torch.float16)


def _bits(t):
    import torch
    return t.detach().cpu().view(torch.int16).numpy().view(np.uint16)


def _finish(*sims):
    for s in sims:
        assert s.device_errors() == 0
        s.close()


def test_the_cases_run_both_kernel_families():
    kernels = {c[6] for c in CASES.values()}
    assert {"step_kernel", "step_kernel_pooled"} <= kernels


# ---------------------------------------------------------------------------------------------- 1. against the two-launch path
@pytest.mark.parametrize("name", list(CASES))
def test_final_positions_equal_the_two_launch_path_bit_for_bit(name, monkeypatch):
    """P: cat_step, keep its team_positions (the terminal tick's own), cat_reset_done.  Q: cat_step_fused(auto_reset=1) with a buffer bound.
    U: the same without one.  Every tick: Q's buffer holds P's kept positions on every row that has ever been terminal -- the latest such
    tick's -- and the sentinel everywhere else; Q's outputs and state equal U's."""
    import torch
    (P, Q, U), tape = _sims(name, monkeypatch, 3)
    A = P.A
    buf = _sentinel(N, A, 2)
    Q.bind_final_positions(buf)
    expected = np.full((N, A, 2), SENTINEL, np.uint16)
    captures = timeouts = 0
    for t in range(12):
        p = to_np(P.step(tape[t]))
        P.reset_done()
        q = to_np(Q.step_fused(tape[t], tick=t, auto_reset=True))
        u = to_np(U.step_fused(tape[t], tick=t, auto_reset=True))
        torch.cuda.synchronize()
        term = p["terminated"] != 0
        assert np.array_equal(q["terminated"] != 0, term), t
        expected[term] = p["team_positions"][term]
        got = _bits(buf)
        assert np.array_equal(got[term], p["team_positions"][term]), (name, t, "terminal rows")
        assert np.array_equal(got, expected), (name, t, "rows that are not terminal were touched")
        assert_outputs_equal(q, u, keys=OUT_KEYS, ctx=f"{name} tick {t}: binding changed an output")
        assert_outputs_equal(q, to_np(P.out), keys=("obs_distance", "obs_type", "shared_distance", "shared_type", "team_positions"), ctx=f"{name} tick {t}: P")
        assert_state_equal(to_np(Q.get_state()), to_np(U.get_state()), ctx=f"{name} tick {t}: binding changed the state")
        captures += int((p["winner"] == 0).sum())
        timeouts += int((p["truncated"] != 0).sum())
    assert captures > 0 and timeouts > 0, (captures, timeouts)
    assert not (expected == SENTINEL).all(axis=(1, 2)).any()          # every slot has ended an episode by tick 6
    _finish(P, Q, U)


# ---------------------------------------------------------------------------------------------- 2. the resident rollout
def _one_tick_rows(sim, tape, T, auto_reset=True):
    """T one-tick launches with a bound [N, A, 2] buffer that is given the sentinel again before every tick: the rows, tick by tick."""
    import torch
    buf = _sentinel(N, sim.A, 2)
    sim.bind_final_positions(buf)
    rows = []
    for t in range(T):
        buf.view(torch.int16).fill_(SENTINEL)
        out = sim.step_fused(tape[t], tick=t, auto_reset=auto_reset)
        rows.append(dict(to_np(out), final_positions=_bits(buf)))
    sim.bind_final_positions(None)
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


@pytest.mark.parametrize("name", [LAB, "labyrinth 2v1 r64 units", "agh-map 2v1 r64 (chunk form)"])
def test_a_resident_rollout_fills_the_rows_of_its_t_n_a_2_buffer(name, monkeypatch):
    import torch
    (one, res), tape = _sims(name, monkeypatch, 2)
    T = 12
    want = _one_tick_rows(one, tape, T)
    buf = _sentinel(T, N, res.A, 2)
    res.bind_final_positions(_sentinel(N, res.A, 2))
    with pytest.raises(ValueError, match="final positions"):           # a one-tick buffer under a resident launch: refused before the launch
        res.rollout_fused(T, tape[:T].contiguous())
    res.bind_final_positions(buf)
    rows = to_np(res.rollout_fused(T, tape[:T].contiguous(), tick=0, auto_reset=True))
    torch.cuda.synchronize()
    term = want["terminated"] != 0
    assert (term.sum(0) >= 2).any(), "no slot ends two episodes inside the launch"
    assert (want["winner"] == 0).any() and (want["truncated"] != 0).any()
    got = _bits(buf)
    assert np.array_equal(got, want["final_positions"]), int((got != want["final_positions"]).sum())
    assert (got[~term] == SENTINEL).all() and not (got[term] == SENTINEL).any()
    for t in range(T):
        assert_outputs_equal({k: v[t] for k, v in rows.items()}, {k: v[t] for k, v in want.items()}, keys=OUT_KEYS, ctx=f"{name} resident tick {t}")
    assert_state_equal(to_np(res.get_state()), to_np(one.get_state()), ctx=f"{name} resident launch")
    _finish(one, res)


# ---------------------------------------------------------------------------------------------- 3. frame skip
@pytest.mark.parametrize("name", [LAB, "labyrinth 2v1 r64 units"])
def test_step_repeat_keeps_the_positions_of_the_tick_that_ended_the_window(name, monkeypatch):
    import torch
    (rep, replay), tape = _sims(name, monkeypatch, 2)
    K = 4
    stagger = torch.arange(N, dtype=torch.int32) % MAX_STEP            # time-outs at every tick of the window
    for s in (rep, replay):
        s.set_state(step_count=stagger)
    held = tape[0]
    rows = _one_tick_rows(replay, held[None].expand(K, -1, -1), K)      # every slot plays all K ticks; the window ends at its first terminal one
    term = rows["terminated"] != 0
    ended = term.any(0)
    jstar = np.where(ended, term.argmax(0), K - 1)
    want = np.where(ended[:, None, None], rows["final_positions"][jstar, np.arange(N)], SENTINEL).astype(np.uint16)
    buf = _sentinel(N, rep.A, 2)
    rep.bind_final_positions(buf)
    out = to_np(rep.step_repeat(held, K, auto_reset=True))
    torch.cuda.synchronize()
    assert (ended & (jstar < K - 1)).any() and (ended & (jstar > 0)).any() and (~ended).any()
    assert (rows["winner"][jstar, np.arange(N)][ended] == 0).any() and (rows["truncated"][jstar, np.arange(N)][ended] != 0).any()
    assert np.array_equal(out["ticks"], jstar + 1) and np.array_equal(out["terminated"] != 0, ended)
    got = _bits(buf)
    assert np.array_equal(got, want), int((got != want).sum())
    assert (got[~ended] == SENTINEL).all()
    _finish(rep, replay)


# ---------------------------------------------------------------------------------------------- 4. / 5. no auto-reset, detach
@pytest.mark.parametrize("name", [LAB, "squarinth 1v1 r90"])
def test_without_auto_reset_terminal_rows_equal_team_positions_and_detach_stops_the_writes(name, monkeypatch):
    import torch
    (sim,), tape = _sims(name, monkeypatch, 1)
    buf = _sentinel(N, sim.A, 2)
    sim.bind_final_positions(buf)
    expected = np.full((N, sim.A, 2), SENTINEL, np.uint16)
    seen = 0
    for t in range(7):
        out = to_np(sim.step(tape[t]) if t % 2 == 0 else sim.step_fused(tape[t], tick=t, auto_reset=False))     # cat_step and cat_step_fused(auto_reset=0)
        term = out["terminated"] != 0
        expected[term] = out["team_positions"][term]
        assert np.array_equal(_bits(buf), expected), (name, t)
        sim.reset_done()                                               # a reset writes nothing
        assert np.array_equal(_bits(buf), expected), (name, t, "cat_reset_done wrote")
        seen += int(term.sum())
    assert seen > N                                                    # the captures of tick 0 and every slot's time-out at tick 5
    # detach: a further tick on which every slot ends leaves the old buffer as it is
    sim.set_state(step_count=torch.full((N,), MAX_STEP - 1, dtype=torch.int32))
    sim.bind_final_positions(None)
    out = to_np(sim.step_fused(tape[7], tick=7, auto_reset=True))
    assert (out["terminated"] != 0).all()
    assert np.array_equal(_bits(buf), expected)
    sim.bind_final_positions(buf)                                      # ... and bound again the next launch writes
    sim.set_state(step_count=torch.full((N,), MAX_STEP - 1, dtype=torch.int32))
    before = to_np(sim.get_state())["pos"]
    out = to_np(sim.step_fused(tape[8], tick=8, auto_reset=True))
    assert np.array_equal(_bits(buf), before.astype(np.float16).view(np.uint16))      # the tick-start body positions themselves
    _finish(sim)


# ---------------------------------------------------------------------------------------------- 6. the tracker
@functools.lru_cache(maxsize=None)
def _rollout_rows():
    """12 ticks of the labyrinth case as one resident launch with a [12, N, A, 2] buffer: the rows both trackers are fed (host copies)."""
    import torch
    from as_cops_and_thieves_amd.sim import CatSim
    cfg, cmap, start, tape = _case(LAB)
    sim = CatSim(cfg, [cmap], device="cuda:0")
    sim.reset(positions=torch.from_numpy(start))
    buf = _sentinel(12, N, sim.A, 2)
    sim.bind_final_positions(buf)
    rows = {k: v.cpu().clone() for k, v in sim.rollout_fused(12, torch.from_numpy(tape[:12]).to("cuda:0"), tick=0, auto_reset=True).items()}
    rows["final_positions"] = buf.cpu().clone()
    assert sim.device_errors() == 0
    sim.close()
    return rows, tuple(int(v) for v in cmap.window)


@pytest.mark.parametrize("quota", [None, 1], ids=["no quota", "quota 1"])
@pytest.mark.parametrize("T", [1, 12])
def test_the_gpu_tracker_equals_the_cpu_tracker_in_every_tensor(T, quota):
    import torch
    from as_cops_and_thieves_amd.positions import CAPTURE, TIMEOUT, PositionTracker
    rows, window = _rollout_rows()
    groups = [(n % 3) - 1 for n in range(N)]                            # -1, 0, 1
    trackers = [PositionTracker(N, ["cop_0", "cop_1", "thief_0"], 2, window, 32, 2, device=d, final_positions=True) for d in ("cpu", "cuda:0")]
    for tr, dev in zip(trackers, ("cpu", "cuda:0")):
        tr.set_groups(groups)
        tr.set_quota(quota)
        r = {k: v.to(dev) for k, v in rows.items()}
        for t0 in range(0, 12, T):
            sl = slice(t0, t0 + T) if T > 1 else t0
            tr.update(r["team_positions"][sl], r["terminated"][sl], r["obs_type"][sl], final_positions=r["final_positions"][sl], truncated=r["truncated"][sl])
    want, got = trackers[0].counts(), trackers[1].counts()
    assert set(got) == set(want) == {"counts", "outside", "rows", "done", "ends", "ends_outside"}
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, int((got[k] != want[k]).sum()))
    ends = want["ends"]
    assert ends[:, CAPTURE].sum() > 0 and ends[:, TIMEOUT].sum() > 0 and want["ends_outside"].sum() == 0
    counted = np.array(groups) >= 0
    term = rows["terminated"].numpy()[:, counted] != 0
    n_ends = int(term.any(0).sum()) if quota == 1 else int(term.sum())
    assert ends.sum() == 3 * n_ends == want["counts"][:, 2].sum()      # one end and one spawn per counted terminal row and agent
    if quota is None:
        assert (term.sum(0) >= 2).any()


# ---------------------------------------------------------------------------------------------- 7. the trainer's captured tick loop
def test_a_captured_tick_loop_of_the_env_replays_with_final_positions_and_maps():
    """Three env ticks -- step_raw, then copies of the rows a learner would keep -- captured in one graph the way the trainer's rollout is,
    replayed three times, against the same twelve ticks played eagerly (three warm-up ticks come first on both sides)."""
    import torch
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    cfg, cmap, start, tape = _case(LAB)
    acts = torch.from_numpy(tape[:3]).to("cuda:0")
    envs = [VecCopsEnv(load_preset("labyrinth", 2, 1), N, num_rays=64, max_step_count=MAX_STEP, seed=29, final_positions=True, track_positions=32)
            for _ in range(2)]
    env, twin = envs
    for e in envs:
        e.reset(options={"positions": torch.from_numpy(start)})
    keep = {k: torch.zeros((3,) + tuple(env.raw_outputs()[k].shape), dtype=env.raw_outputs()[k].dtype, device="cuda:0")
            for k in ("final_positions", "terminated", "truncated", "team_positions")}

    def loop(e, into):
        for j in range(3):
            out = e.step_raw(acts[j])
            for k, v in into.items():
                v[j].copy_(out[k])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # warm-up on the side stream, as torch's capture wants it
        loop(env, keep)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loop(env, keep)
    replayed = []
    for _ in range(3):
        graph.replay()
        replayed.append({k: v.clone() for k, v in keep.items()})
    eager_keep = {k: torch.zeros_like(v) for k, v in keep.items()}
    loop(twin, eager_keep)
    eager = []
    for _ in range(3):
        loop(twin, eager_keep)
        eager.append({k: v.clone() for k, v in eager_keep.items()})
    torch.cuda.synchronize()
    ends = 0
    for r, (a, b) in enumerate(zip(replayed, eager)):
        for k in a:
            assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), (r, k)
        ends += int(a["terminated"].sum())
    assert ends >= N                                        # every slot times out once in ticks 4 .. 12
    assert env.raw_outputs()["final_positions"].data_ptr() == env._final_pos.data_ptr()
    got, want = env.position_tracker.counts(), twin.position_tracker.counts()
    for k in ("counts", "ends", "ends_outside", "outside", "rows", "done"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["ends"][:, 0].sum() > 0 and got["ends"][:, 1].sum() > 0 and got["rows"][0] == 12 * N
    s = env.position_stats()[0]["agents"]["thief_0"]
    assert s["captures"] + s["timeouts"] == int(got["ends"][0, :, 2].sum()) and s["top_timeout_cell"] is not None
    _, _, _, _, infos = env.step(acts[0])
    assert infos["final_positions"].data_ptr() == env._final_pos.data_ptr() and infos["final_positions"].dtype == torch.float16
    for e in envs:
        e.check_errors()
        e.close()
