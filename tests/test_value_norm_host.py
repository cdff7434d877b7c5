"""Running value normalisation (``TrainerConfig.value_norm``; include/cat_ppo.h: cat_ppo_gae_scan_scaled, cat_ppo_moments) as far as a host
without a device can see it: header <-> binding table <-> ctypes mirrors, the entries' argument checks, the package's CPU restatement of
the moments against THIS file's own NumPy restatement (written from the header, loops and Python floats, nothing imported from the
package), and the learner's CPU path: state after updates, checkpoints, the option off, and two gloo ranks.

``np_moments`` / ``np_merge`` / ``np_scale`` below are also what tests/test_gpu_value_norm.py holds the kernels to, bit for bit."""
import ctypes as C
import math
import os
import re
import socket
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parents[1]
MOMENT_SIZES = (1, 255, 256, 4095, 4096, 4097, 3 * 4096 + 5, 5 * 4096)      # the last: five chunks padded to eight
MOMENT_AGENTS = (1, 3, 8)


# ---------------------------------------------------------------------------------------------- the header's order, restated
def np_merge(a, b):
    """merge(a, b) of two (n, mean, M2) triples of Python floats (IEEE f64, one rounding per operation)."""
    if b[0] == 0.0:
        return a
    if a[0] == 0.0:
        return b
    n = a[0] + b[0]
    delta = b[1] - a[1]
    w = b[0] / n
    mean = a[1] + delta * w
    m2 = (a[2] + b[2]) + (delta * delta) * (a[0] * w)
    return (n, mean, m2)


def _np_chunk(x):
    """One chunk (fp32, at most 4096 elements) -> (n_c, mean_c, M2_c): 256 threads, 16 strided elements each, a halving tree."""
    count = len(x)
    lane = np.arange(256)

    def total(e):
        s = np.zeros(256, np.float64)
        for j in range(16):
            k = lane + 256 * j
            ok = k < count
            s[ok] = s[ok] + e[k[ok]]
        stride = 128
        while stride:
            s[:stride] = s[:stride] + s[stride:2 * stride]
            stride //= 2
        return float(s[0])
    v = x.astype(np.float64)
    n = float(count)
    mean = total(v) / n
    d = v - mean
    return (n, mean, total(d * d))


def np_moments(x):
    """x fp32 [G, M] -> f64 [G, 3]: the batch moments of every row in cat_ppo_moments's order."""
    out = np.zeros((x.shape[0], 3), np.float64)
    for g, row in enumerate(np.asarray(x, np.float32)):
        t = [_np_chunk(row[c:c + 4096]) for c in range(0, len(row), 4096)]
        P = 1
        while P < len(t):
            P *= 2
        t += [(0.0, 0.0, 0.0)] * (P - len(t))
        stride = P // 2
        while stride:
            for i in range(stride):
                t[i] = np_merge(t[i], t[i + stride])
            stride //= 2
        out[g] = t[0]
    return out


def np_merge_rows(state, batch):
    return np.array([np_merge(tuple(map(float, a)), tuple(map(float, b))) for a, b in zip(state, batch)], np.float64).reshape(-1, 3)


def np_scale(state):
    """f64 [G, 3] -> fp32 [G, 2] = (mu, sigma), (0, 1) while n == 0."""
    return np.array([(np.float32(0.0), np.float32(1.0)) if n == 0.0 else (np.float32(mean), np.float32(np.sqrt(np.float64(m2) / np.float64(n))))
                     for n, mean, m2 in state], np.float32).reshape(-1, 2)


def moment_inputs(G, M, seed=0):
    """Seeded fp32 [G, M] with a mean far from zero and a different spread per agent (what returns look like)."""
    rng = np.random.default_rng(1000 * G + M + seed)
    return (rng.standard_normal((G, M)) * (1.0 + np.arange(G)[:, None]) * 3.0 + 11.0 * (1 + np.arange(G)[:, None])).astype(np.float32)


# ---------------------------------------------------------------------------------------------- ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_ppo.h").read_text(), flags=re.S)


def _fields(code, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, re.S).group(1)
    return [n for decl in body.split(";") for n in re.findall(r"\b([A-Za-z_0-9]+)\s*(?=,|$)", decl.strip())]


def test_header_table_and_mirrors_agree():
    from as_cops_and_thieves_amd import _learn_native as ln
    ln.build()
    L = ln.lib()
    code = _header()
    declared = set(re.findall(r"\b(cat_ppo_[a-z_0-9]+)\s*\(", code))
    new = {"cat_ppo_gae_scan_scaled", "cat_ppo_moments", "cat_ppo_moment_chunks"}
    assert new <= declared and declared == set(ln.PPO_SYMBOLS) and all(hasattr(L, s) for s in declared)
    assert new <= set(ln.MODULES["cat_ppo"][1]) and ln.MODULES["cat_ppo"][0] == 2 and L.cat_ppo_abi_version() == 2
    assert _fields(code, "cat_ppo_gae_scaled") == [f[0].rstrip("_") for f in ln.PpoGaeScaled._fields_]
    assert _fields(code, "cat_ppo_gae_scaled")[:-1] == _fields(code, "cat_ppo_gae") and _fields(code, "cat_ppo_gae_scaled")[-1] == "scale"
    assert [f[1] for f in ln.PpoGaeScaled._fields_[:-1]] == [f[1] for f in ln.PpoGae._fields_]
    assert _fields(code, "cat_ppo_moments_args") == [f[0] for f in ln.PpoMoments._fields_]
    assert C.sizeof(ln.PpoMoments) == 8 + 5 * 8 and C.sizeof(ln.PpoGaeScaled) == C.sizeof(ln.PpoGae) + 8
    assert re.search(r"#define CAT_PPO_MOMENT_CHUNK 4096\b", code) and ln.PPO_MOMENT_CHUNK == 4096
    assert [ln.ppo_moment_chunks(M) for M in (1, 4096, 4097)] == [1, 1, 2]


def test_entries_reject_bad_arguments_before_any_device_call():
    """No device here: a call that got past its checks would fail in the runtime (-2) or worse, not return -1 with a message."""
    from as_cops_and_thieves_amd import _learn_native as ln
    L = ln.lib()
    p = 4096                                     # a non-NULL address that no check dereferences
    err = lambda: L.cat_ppo_last_error().decode()
    assert L.cat_ppo_gae_scan_scaled(None, None) == -1 and L.cat_ppo_moments(None, None) == -1
    assert L.cat_ppo_gae_scan_scaled(C.byref(ln.PpoGaeScaled()), None) == -1 and "cat_ppo_gae_scan_scaled: bad dimensions" in err()
    for dims in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        assert L.cat_ppo_gae_scan_scaled(C.byref(ln.PpoGaeScaled(*dims, 0, p, p, p, p, 0.99, 0.95, p, p, p)), None) == -1 and "dimensions" in err()
    for missing in range(7):                     # each of the seven buffers in turn, scale among them
        ptrs = [None if i == missing else p for i in range(7)]
        a = ln.PpoGaeScaled(2, 4, 4, 0, ptrs[0], ptrs[1], ptrs[2], ptrs[3], 0.99, 0.95, ptrs[4], ptrs[5], ptrs[6])
        assert L.cat_ppo_gae_scan_scaled(C.byref(a), None) == -1 and "NULL" in err(), missing
    assert L.cat_ppo_moments(C.byref(ln.PpoMoments()), None) == -1 and "cat_ppo_moments: bad dimensions" in err()
    assert L.cat_ppo_moments(C.byref(ln.PpoMoments(0, 5, p, p, None, None, None)), None) == -1 and "dimensions" in err()
    assert L.cat_ppo_moments(C.byref(ln.PpoMoments(2, 0, p, p, None, None, None)), None) == -1 and "dimensions" in err()
    assert L.cat_ppo_moments(C.byref(ln.PpoMoments(2, 5, None, p, None, None, None)), None) == -1 and "NULL" in err()
    assert L.cat_ppo_moments(C.byref(ln.PpoMoments(2, 5, p, None, None, None, None)), None) == -1 and "NULL" in err()
    assert L.cat_ppo_moments(C.byref(ln.PpoMoments(2, 5, p, p, None, None, p)), None) == -1 and "scale_out needs state" in err()
    assert L.cat_ppo_moments(C.byref(ln.PpoMoments(1, 65536 * 4096 + 1, p, p, None, None, None)), None) == -1 and "65536 chunks" in err()
    assert [L.cat_ppo_moment_chunks(M) for M in (-3, 0, 1, 4096, 4097, 65536 * 4096, 65536 * 4096 + 1)] == [0, 0, 1, 1, 2, 65536, 65537]
    with pytest.raises(ValueError):
        ln.ppo_moments(torch.zeros(2, 5), scale_out=torch.zeros(2, 2))


# ---------------------------------------------------------------------------------------------- the CPU restatement
@pytest.mark.parametrize("G", MOMENT_AGENTS)
@pytest.mark.parametrize("M", MOMENT_SIZES)
def test_cpu_restatement_equals_the_numpy_restatement_bit_for_bit(G, M):
    from as_cops_and_thieves_amd.selfplay import mappo
    x = moment_inputs(G, M)
    want = np_moments(x)
    got = mappo.running_moments(torch.from_numpy(x))
    assert got.dtype == torch.float64 and got.shape == (G, 3)
    assert np.array_equal(got.numpy().view(np.uint64), want.view(np.uint64)), (got, want)
    for g in range(G):          # sanity against the exactly rounded sum: far inside M * 2^-52 * max|x|
        exact = math.fsum(float(v) for v in x[g]) / M
        assert want[g, 0] == M and abs(want[g, 1] - exact) <= M * 2.0 ** -52 * float(np.abs(x[g]).max())
        assert abs(want[g, 2] - math.fsum((float(v) - exact) ** 2 for v in x[g])) <= 1e-9 * max(want[g, 2], 1.0)
    # a second batch into the state, and the scale: merge and (mu, sigma) of the package against this file's
    y = moment_inputs(G, M, seed=7)
    state = mappo.merge_moments(mappo.merge_moments(torch.zeros(G, 3, dtype=torch.float64), got), mappo.running_moments(torch.from_numpy(y)))
    want_state = np_merge_rows(np_merge_rows(np.zeros((G, 3)), want), np_moments(y))
    assert np.array_equal(state.numpy().view(np.uint64), want_state.view(np.uint64))
    assert np.array_equal(mappo.moments_scale(state).numpy().view(np.uint32), np_scale(want_state).view(np.uint32))
    fresh = mappo.moments_scale(torch.zeros(G, 3, dtype=torch.float64))
    assert fresh.dtype == torch.float32 and fresh.tolist() == [[0.0, 1.0]] * G
    if M == 1:                  # one sample: sigma 0, mu that element
        one = mappo.moments_scale(got)
        assert one[:, 1].tolist() == [0.0] * G and np.array_equal(one[:, 0].numpy(), x[:, 0])


# ---------------------------------------------------------------------------------------------- the learner on the CPU
def _env(n=6, seed=1, off=0):
    from as_cops_and_thieves_amd.maps import load_preset
    from tests.fake_env import OracleVecEnv
    return OracleVecEnv(load_preset("squarinth").compile(), n, num_rays=16, max_step_count=12, seed=seed, env_id_offset=off)


def _trainer(seed=0, n=6, off=0, **tc_kw):
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
    rc = RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=0, learning_starts=0, learning_rate=3e-3)
    tc = TrainerConfig(horizon=4, policy_freeze_duration=0, opponent_freeze_duration=0, **tc_kw)
    return MAPPOTrainer(_env(n, off=off), {"cop": rc, "thief": rc}, tc, seed=seed)


def _record_moment_inputs(rl, into):
    inner = rl._moments_step

    def wrapped(raw):
        into.append(raw.detach().cpu().numpy().copy())
        return inner(raw)
    rl._moments_step = wrapped


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint64)


def _same_models(a, b):
    """every agent's policy and value parameters, by the reference modules' names"""
    return all(torch.equal(v, b.agent_models(ag)[kind][n]) for ag in a.agents for kind, sd in a.agent_models(ag).items() for n, v in sd.items())


def test_cpu_trainer_state_follows_the_restatement_and_survives_a_checkpoint():
    tr = _trainer(value_norm=True)
    (rl,) = tr.roles.values()
    assert rl.vn_state.dtype == torch.float64 and rl.vn_state.shape == (rl.G, 3) and not rl.vn_state.any()
    assert rl.vn_scale.dtype == torch.float32 and rl.vn_scale.tolist() == [[0.0, 1.0]] * rl.G
    stats0 = tr.read_stats()
    assert all(stats0[f"value_mean/{a}"] == 0.0 and stats0[f"value_std/{a}"] == 1.0 for a in tr.agents)
    seen = []
    _record_moment_inputs(rl, seen)
    want = np.zeros((rl.G, 3))
    for k in range(2):
        tr.collect(); tr.update()
        assert len(seen) == k + 1 and seen[k].shape == (rl.G, 4 * 6) and seen[k].dtype == np.float32
        want = np_merge_rows(want, np_moments(seen[k]))
        assert np.array_equal(_bits(rl.vn_state), want.view(np.uint64)), k
        assert np.array_equal(rl.vn_scale.numpy().view(np.uint32), np_scale(want).view(np.uint32))
        # the critic's targets: the raw returns handed to the moments step, normalised with the scale that followed
        mu, sigma = rl.vn_scale[:, :1], rl.vn_scale[:, 1:]
        assert torch.equal(rl.buf["ret"].view(rl.G, -1), (torch.from_numpy(seen[k]) - mu) / (sigma + 1e-8))
    assert float(want[0, 0]) == 2 * 4 * 6 and rl.vn_scale.tolist() != [[0.0, 1.0]] * rl.G
    stats = tr.read_stats()
    for g, a in enumerate(tr.agents):
        assert stats[f"value_mean/{a}"] == float(rl.vn_scale[g, 0]) and stats[f"value_std/{a}"] == float(rl.vn_scale[g, 1])
        assert math.isfinite(stats[f"value_mean/{a}"]) and stats[f"value_std/{a}"] > 0.0
    # state_dict -> a fresh trainer -> load_state_dict: bit-equal state, scale and models
    sd = tr.state_dict()
    assert all(sd[a]["vn_state"].dtype == torch.float64 and sd[a]["vn_state"].shape == (3,) for a in tr.agents)
    tr2 = _trainer(seed=5, value_norm=True)
    (rl2,) = tr2.roles.values()
    tr2.load_state_dict(sd)
    assert np.array_equal(_bits(rl2.vn_state), _bits(rl.vn_state)) and torch.equal(rl2.vn_scale, rl.vn_scale)
    assert _same_models(tr, tr2)
    # a checkpoint without the key loads as a fresh scaler
    old = {a: {k: v for k, v in e.items() if k != "vn_state"} if a in tr.agents else e for a, e in sd.items()}
    tr2.load_state_dict(old)
    assert not rl2.vn_state.any() and rl2.vn_scale.tolist() == [[0.0, 1.0]] * rl2.G and _same_models(tr, tr2)
    # ... and one with the key into a trainer without the option: ignored, one warning
    tr3 = _trainer(seed=5)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        tr3.load_state_dict(sd)
    assert len([w for w in caught if "vn_state" in str(w.message)]) == 1
    assert _same_models(tr, tr3) and not hasattr(next(iter(tr3.roles.values())), "vn_state")
    assert "vn_state" not in tr3.state_dict()[tr.agents[0]]


def test_a_frozen_critic_keeps_its_moments_and_scale():
    """While an agent's value network is frozen its critic is not trained, so its rows of ``vn_state`` / ``vn_scale`` stay as they are; the
    other agents' rows follow the restatement, and after the release the agent takes in the batches from then on."""
    tr = _trainer(value_norm=True)
    (rl,) = tr.roles.values()
    thief, cops = rl.rows("thief"), rl.rows("cop")
    assert thief and cops
    seen = []
    _record_moment_inputs(rl, seen)
    tr.set_frozen(role="thief", value=True)
    want = np.zeros((rl.G, 3))
    for k in range(2):
        tr.collect(); tr.update()
        merged = np_merge_rows(want, np_moments(seen[k]))
        want[cops] = merged[cops]
        assert np.array_equal(_bits(rl.vn_state), want.view(np.uint64)), k
        assert np.array_equal(rl.vn_scale.numpy().view(np.uint32), np_scale(want).view(np.uint32))
    assert not want[thief].any() and rl.vn_scale[thief].tolist() == [[0.0, 1.0]] * len(thief) and want[cops, 0].tolist() == [48.0] * len(cops)
    tr.set_frozen(role="thief", value=False)
    tr.collect(); tr.update()
    want = np_merge_rows(want, np_moments(seen[2]))
    assert np.array_equal(_bits(rl.vn_state), want.view(np.uint64)) and want[thief, 0].tolist() == [24.0] * len(thief)
    assert np.array_equal(rl.vn_scale.numpy().view(np.uint32), np_scale(want).view(np.uint32))


def test_option_off_is_the_default_and_adds_nothing():
    from as_cops_and_thieves_amd.selfplay.mappo import TrainerConfig
    assert TrainerConfig().value_norm is False
    digests = []
    for kw in ({"value_norm": False}, {}, {"value_norm": True}):     # one after the other: a trainer seeds the global generator it samples from
        tr = _trainer(**kw)
        for _ in range(2):
            tr.collect(); tr.update()
        digests.append(tr.param_digest())
        (rl,) = tr.roles.values()
        if not kw.get("value_norm"):
            assert not rl.value_norm and not hasattr(rl, "vn_state") and not hasattr(rl, "vn_scale")
            assert not any(k.startswith("value_mean/") or k.startswith("value_std/") for k in tr.read_stats())
    assert digests[0] == digests[1]
    assert digests[2] != digests[0]                         # the option does change what the critic is trained on


def _rank_worker(rank, world, port, q):
    sys.path.insert(0, str(ROOT))
    warnings.filterwarnings("ignore")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    tr = _trainer(n=4, off=4 * rank, value_norm=True)
    (rl,) = tr.roles.values()
    seen = []
    _record_moment_inputs(rl, seen)
    tr.collect(); tr.update()
    q.put((rank, seen[0], rl.vn_state.numpy().copy(), rl.vn_scale.numpy().copy(), tr.param_digest()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_hold_the_rank_order_merge_of_their_shards():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, rest) for r, *rest in (q.get(timeout=300) for _ in range(2)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (x0, s0, c0, d0), (x1, s1, c1, d1) = got[0], got[1]
    assert not np.array_equal(x0, x1)                        # the shards really differ
    assert np.array_equal(s0.view(np.uint64), s1.view(np.uint64)) and np.array_equal(c0.view(np.uint32), c1.view(np.uint32)) and d0 == d1
    want = np_merge_rows(np_merge_rows(np.zeros_like(s0), np_moments(x0)), np_moments(x1))
    assert np.array_equal(s0.view(np.uint64), want.view(np.uint64)) and np.array_equal(c0.view(np.uint32), np_scale(want).view(np.uint32))
