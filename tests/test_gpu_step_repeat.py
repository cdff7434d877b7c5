"""cat_step_repeat (frame skip): k held-action ticks per env slot in one resident launch, against the one-tick entry.

Scheme of every case: two sims created alike.  Sim A gets one ``step_repeat(actions, k)`` per decision, sim B k single ``step_fused`` calls
with the same action row, every output and the whole state snapshotted after each.  Slot n is expected to hold B's snapshot at j*(n), the first
tick whose ``terminated[n]`` is set (else k - 1), the fp32 left fold of B's reward rows 0 .. j*(n) and ``ticks`` = j* + 1.  After a decision
the expected state is written into B, which puts the slots that ran on past j* back where A holds them.  Everything is compared bit for bit.

The mid-window cases start the slots at DIFFERENT phases of their episodes (``step_count`` = slot index mod ``max_step_count``, set in both
sims): with every slot in phase, a time-out ends all episodes at the same tick and they stay in phase for ever, so no two slots of a
workgroup could stop at different ticks.  With ``max_step_count`` = 6 a window of k = 7 ticks always contains a time-out before its last tick:
"ended at j* = k - 1" and "did not end" cannot occur there, and are asserted for k = 2 and k = 4 only.
"""
import ctypes as C

import numpy as np
import pytest

from tests.util import OUT_KEYS, assert_outputs_equal, assert_state_equal, to_np

pytestmark = pytest.mark.gpu

SHAPES = {"labyrinth": ("labyrinth", 2, 1, 64), "agh-map": ("agh-map", 2, 1, 64), "3v2": ("grandbyrinth", 3, 2, 90)}
MAX_STEP = 6


def _maps(name, cops, thieves):
    from as_cops_and_thieves_amd.maps import load_preset
    return [load_preset(name, cops, thieves).compile()]


def _twins(shape, N, max_step=MAX_STEP, seed=41, maps=None, slot=None):
    from as_cops_and_thieves_amd.config import SimConfig
    from as_cops_and_thieves_amd.sim import CatSim
    name, cops, thieves, rays = SHAPES[shape]
    cfg = lambda: SimConfig(n_envs=N, n_cops=cops, n_thieves=thieves, n_rays=rays, max_step_count=max_step, seed=seed, env_id_offset=1000)
    maps = maps or _maps(name, cops, thieves)
    a, b = (CatSim(cfg(), maps, slot, device="cuda:0", debug_hit_shape=True) for _ in range(2))
    a.reset(); b.reset()
    return a, b


def _stagger(a, b, period=MAX_STEP):
    import torch
    sc = (torch.arange(a.N, dtype=torch.int32) % period).to(a.device)
    a.set_state(step_count=sc); b.set_state(step_count=sc)


def _snapshot(sim):
    import torch
    torch.cuda.synchronize()
    return to_np(sim.out), to_np(sim.get_state())


def _expected(b, actions, k, auto_reset=True, rows_out=None):
    """k one-tick launches of B -> (expected outputs incl. ticks, expected state, j* [N], ended [N]).  ``rows_out``: a list that
    receives B's k output rows."""
    import torch
    rows, states = [], []
    for _ in range(k):
        b.step_fused(actions, auto_reset=auto_reset)
        o, s = _snapshot(b)
        rows.append(o); states.append(s)
    if rows_out is not None:
        rows_out.extend(rows)
    N = b.N
    term = np.stack([r["terminated"] for r in rows]) != 0
    ended = term.any(0)
    jstar = np.where(ended, term.argmax(0), k - 1)
    pick = lambda seq: np.stack(seq)[jstar, np.arange(N)]
    out = {key: pick([r[key] for r in rows]) for key in rows[0] if key != "reward"}
    acc = torch.from_numpy(rows[0]["reward"].copy())                     # the fp32 left fold, one add at a time
    for j in range(1, k):
        nxt = acc + torch.from_numpy(rows[j]["reward"])
        acc = torch.where(torch.from_numpy(jstar >= j)[:, None], nxt, acc)
    out["reward"] = acc.numpy()
    out["ticks"] = (jstar + 1).astype(np.int32)
    state = {key: pick([s[key] for s in states]) for key in states[0]}
    return out, state, jstar, ended


def _decide(a, b, actions, k, ctx, auto_reset=True):
    import torch
    a.step_repeat(actions, k, auto_reset=auto_reset)
    want, state, jstar, ended = _expected(b, actions, k, auto_reset)
    got, got_state = _snapshot(a)
    assert_outputs_equal(got, want, keys=OUT_KEYS + ("ticks",), ctx=ctx)
    assert "hit_shape" in got and "ticks" in got
    assert_state_equal(got_state, state, ctx=ctx)
    b.set_state(**{key: torch.from_numpy(np.ascontiguousarray(v)) for key, v in state.items()})
    return want, state, jstar, ended


def _actions(rng, sim):
    import torch
    return torch.from_numpy(rng.integers(0, 4, size=(sim.N, sim.A), dtype=np.int32)).to(sim.device)


@pytest.mark.parametrize("k", [2, 4, 7])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_windows_with_episode_ends_inside_them(shape, k):
    a, b = _twins(shape, 70)
    _stagger(a, b)
    rng = np.random.default_rng(100 * k + len(shape))
    early = at_end = none = split = False
    for d in range(6):
        _, _, jstar, ended = _decide(a, b, _actions(rng, a), k, f"{shape} k={k} decision {d}")
        early |= bool((ended & (jstar < k - 1)).any())
        at_end |= bool((ended & (jstar == k - 1)).any())
        none |= bool((~ended).any())
        split |= bool(jstar[0] != jstar[1])      # slots 0 and 1 share a workgroup whenever a workgroup holds more than one slot
    assert early and split, (early, split)
    if k <= MAX_STEP:
        assert at_end and none, (at_end, none)
    assert a.device_errors() == 0 and b.device_errors() == 0
    a.close(); b.close()


def test_both_schedulers_are_covered():
    from as_cops_and_thieves_amd.config import SimConfig
    from as_cops_and_thieves_amd.sim import CatSim
    names = set()
    for name, cops, thieves, rays in SHAPES.values():
        sim = CatSim(SimConfig(n_envs=70, n_cops=cops, n_thieves=thieves, n_rays=rays, seed=1), _maps(name, cops, thieves), device="cuda:0")
        names.add(sim.rollout_kernel)
        sim.close()
    assert "rollout_kernel_pooled" in names and "rollout_kernel" in names, names


def test_single_slot_batch():
    a, b = _twins("labyrinth", 1)
    rng = np.random.default_rng(5)
    ticks = []
    for d in range(4):
        want, _, _, _ = _decide(a, b, _actions(rng, a), 4, f"N=1 decision {d}")
        ticks.append(int(want["ticks"][0]))
    assert all(1 <= t <= 4 for t in ticks) and min(ticks) < 4, ticks      # an episode lasts six ticks at most: some window is cut short
    assert a.device_errors() == 0
    a.close(); b.close()


def test_five_map_batch():
    from as_cops_and_thieves_amd.maps import load_preset
    maps = [load_preset(n, 2, 1).compile() for n in ("squarinth", "lbirinth", "labyrinth", "grandbyrinth", "agh-map")]
    slot = (np.arange(40) * 3 % 5).astype(np.int32)
    a, b = _twins("labyrinth", 40, maps=maps, slot=slot)
    _stagger(a, b)
    rng = np.random.default_rng(9)
    for d in range(4):
        _decide(a, b, _actions(rng, a), 4, f"five maps decision {d}")
    assert a.device_errors() == 0
    a.close(); b.close()


def test_capture_inside_a_window():
    """A thief placed inside the capture distance of cop 0 (clear of walls, line of sight open) in every third slot: those slots stop after their first
    tick with the cops' win, and their new episode is not stepped."""
    import torch
    from as_cops_and_thieves_amd.config import SimConfig
    from oracle.cat_oracle import OracleSim
    a, b = _twins("labyrinth", 72, max_step=400)
    name, cops, thieves, rays = SHAPES["labyrinth"]
    m = _maps(name, cops, thieves)
    probe = OracleSim(SimConfig(n_envs=72, n_cops=cops, n_thieves=thieves, n_rays=rays, max_step_count=400, seed=41, env_id_offset=1000), m)
    probe.reset()
    pos = to_np(a.get_state())["pos"].copy()
    forced = np.arange(72) % 3 == 0
    for e in np.nonzero(forced)[0]:
        for ang in np.arange(16) * (np.pi / 8):
            p = pos[e, 0] + 15.0 * np.array([np.cos(ang), np.sin(ang)])      # between the two radii (10) and the capture distance (20)
            if not probe.point_query_any(int(e), -2, p, 6.5):
                pos[e, 2] = p
                break
        else:
            raise RuntimeError("no free spot beside cop 0")
    a.reset(positions=torch.from_numpy(pos)); b.reset(positions=torch.from_numpy(pos))
    rng = np.random.default_rng(3)
    want, state, jstar, ended = _decide(a, b, _actions(rng, a), 4, "capture")
    assert (want["ticks"][forced] == 1).all() and (want["winner"][forced] == 0).all() and (jstar[forced] == 0).all()
    assert (state["step_count"][forced] == 0).all() and (state["reset_count"][forced] == state["reset_count"][~forced].min() + 1).all()
    assert (want["ticks"][~forced] == 4).sum() > 0
    assert a.device_errors() == 0
    a.close(); b.close()


def test_k_1_is_the_one_tick_entry():
    a, b = _twins("labyrinth", 70)
    _stagger(a, b)
    rng = np.random.default_rng(1)
    for d in range(3):
        want, _, _, _ = _decide(a, b, _actions(rng, a), 1, f"k=1 decision {d}")
        assert (want["ticks"] == 1).all()
    a.close(); b.close()


def test_without_auto_reset_a_held_slot_stays_as_the_terminal_tick_left_it():
    a, b = _twins("agh-map", 70, max_step=2)
    rng = np.random.default_rng(2)
    want, state, jstar, ended = _decide(a, b, _actions(rng, a), 4, "no auto-reset", auto_reset=False)
    assert ended.all() and (jstar == 1).all() and (state["step_count"] == 2).all() and (want["truncated"] == 1).all()
    a.close(); b.close()


def _raw_call(sim, k, actions_ptr, out_struct, ticks_ptr, auto_reset=1):
    return sim._L.cat_step_repeat(sim._h, k, actions_ptr, auto_reset, None if out_struct is None else C.byref(out_struct), ticks_ptr, sim._stream())


def test_null_outputs_still_advance_the_state():
    a, b = _twins("labyrinth", 70)
    _stagger(a, b)
    acts = _actions(np.random.default_rng(4), a)
    assert _raw_call(a, 4, acts.data_ptr(), None, None) == 0
    _, state, _, _ = _expected(b, acts, 4)
    assert_state_equal(to_np(a.get_state()), state, ctx="NULL outputs")
    assert a.device_errors() == 0
    a.close(); b.close()


def test_guarded_buffers_are_untouched_outside_their_rows():
    import torch
    from as_cops_and_thieves_amd import _native as nat
    from as_cops_and_thieves_amd.sim import _OUT_SPEC
    a, b = _twins("3v2", 70)
    _stagger(a, b)
    acts = _actions(np.random.default_rng(6), a)
    M = 512
    raw, ptrs = {}, []
    for key in nat.OUT_FIELDS + ("ticks",):
        shape, dt = ((a.N,), torch.int32) if key == "ticks" else (_OUT_SPEC[key][0](a.N, a.A, a.R), _OUT_SPEC[key][1])
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        raw[key] = (torch.full((nbytes + 2 * M,), 0xA5, dtype=torch.uint8, device=a.device), nbytes, shape, dt)
        ptrs.append(raw[key][0].data_ptr() + M)
    assert _raw_call(a, 4, acts.data_ptr(), nat.CatOutputs(*ptrs[:-1]), ptrs[-1]) == 0
    want, state, _, _ = _expected(b, acts, 4)
    torch.cuda.synchronize()
    got = {}
    for key, (buf, nbytes, shape, dt) in raw.items():
        assert bool((buf[:M] == 0xA5).all()) and bool((buf[M + nbytes:] == 0xA5).all()), f"{key}: written outside [N, ...]"
        got[key] = buf[M:M + nbytes].view(dt).reshape(shape)
    assert_outputs_equal(to_np(got), want, keys=OUT_KEYS + ("ticks",), ctx="guarded")
    assert_state_equal(to_np(a.get_state()), state, ctx="guarded")
    a.close(); b.close()


def test_argument_errors_come_back_as_codes_without_a_launch():
    from as_cops_and_thieves_amd import _native as nat
    from as_cops_and_thieves_amd.sim import CatSimError
    a, b = _twins("labyrinth", 8)
    before = to_np(a.get_state())
    acts = _actions(np.random.default_rng(7), a)
    for k, ptr, text in ((0, acts.data_ptr(), b"k = 0"), (nat.MAX_ROLLOUT_TICKS + 1, acts.data_ptr(), b"outside"), (4, None, b"actions is NULL")):
        assert _raw_call(a, k, ptr, a._out_struct, None) == -6
        assert text in a._L.cat_last_error(a._h)
    with pytest.raises(CatSimError):
        a.step_repeat(acts, 0)
    with pytest.raises(ValueError):
        a.step_repeat(acts, 2.5)
    assert_state_equal(to_np(a.get_state()), before, ctx="rejected calls")
    assert a.device_errors() == 0
    a.close(); b.close()


def test_bad_action_is_flagged_and_applied_as_in_the_one_tick_entry():
    from as_cops_and_thieves_amd import _native as nat
    a, b = _twins("labyrinth", 70)
    _stagger(a, b)
    acts = _actions(np.random.default_rng(8), a)
    acts[33, 1] = 7
    _decide(a, b, acts, 4, "bad action")
    assert a.device_errors() == nat.DEVERR_BAD_ACTION and b.device_errors() == nat.DEVERR_BAD_ACTION
    a.close(); b.close()


def test_graph_capture_of_a_repeat_step():
    import torch
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    mk = lambda: VecCopsEnv(load_preset("labyrinth", 2, 1), 70, max_step_count=MAX_STEP, seed=12, device="cuda:0")
    ea, eb = mk(), mk()
    ea.reset(); eb.reset()
    rng = np.random.default_rng(11)
    acts = _actions(rng, ea._sim)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture (creates the ticks tensor); the twin takes the same call
        ea.step_raw(acts, repeat=4)
    torch.cuda.current_stream().wait_stream(side)
    eb.step_raw(acts, repeat=4)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ea.step_raw(acts, repeat=4)
    for r in range(3):
        new = _actions(rng, ea._sim)
        acts.copy_(new)
        g.replay()
        out_b = eb.step_raw(new, repeat=4)
        torch.cuda.synchronize()
        assert_outputs_equal(to_np(ea.raw_outputs()), to_np(out_b), keys=OUT_KEYS + ("ticks",), ctx=f"replay {r}")
        assert_state_equal(to_np(ea.get_env_state()), to_np(eb.get_env_state()), ctx=f"replay {r}")
    ea.check_errors(); eb.check_errors()
    ea.close(); eb.close()
