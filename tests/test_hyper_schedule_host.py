"""Learner schedules on the device (``RoleConfig.lr_schedule`` / ``entropy_final`` / ``ratio_clip_final``; include/cat_ppo.h: the hyper block,
cat_ppo_loss_grad_dev, cat_ppo_adam_step_dev, cat_ppo_schedule_step) as far as a host without a device can see them: header <-> binding
table <-> ctypes mirrors, the entries' argument checks, the package's CPU restatement of the schedule rule against THIS file's own NumPy
restatement (written from the header: one ``np.float32`` operation per line, nothing imported from the package) and against hand-written
known answers, and the learner's CPU path: the option off, the rule's effect on the learning rates, frozen policies, checkpoints.

``np_schedule``, ``kl_table`` and ``ANNEAL_CASES`` below are also what tests/test_gpu_hyper_schedule.py holds the kernel to, bit for bit."""
import ctypes as C
import dataclasses
import re
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
F = np.float32
LR, ENTROPY, RATIO_CLIP, KL_SUM, KL_COUNT, STRIDE = 0, 1, 2, 3, 4, 8
SCHED_KL, SCHED_ANNEAL = 1, 2
KL_ARGS = dict(kl_target=0.008, kl_factor=2.0, lr_factor=1.5, lr_min=1e-6, lr_max=1e-2)


# ---------------------------------------------------------------------------------------------- the header's rule, restated
def np_schedule(hyper, active, mode, kl_target=0.008, kl_factor=2.0, lr_factor=1.5, lr_min=1e-6, lr_max=1e-2, anneal_mask=0, progress=0.0,
                lr=(0.0, 0.0), entropy=(0.0, 0.0), ratio_clip=(0.0, 0.0)):
    """hyper fp32 [G, 8], active fp32 [G] -> the block after cat_ppo_schedule_step (a copy); agent by agent, one rounded operation per line."""
    h = np.array(hyper, np.float32)
    assert h.dtype == np.float32 and h.shape[1] == STRIDE
    for g in range(h.shape[0]):
        if mode & SCHED_ANNEAL:
            for bit, col, (x0, x1) in ((1, LR, lr), (2, ENTROPY, entropy), (4, RATIO_CLIP, ratio_clip)):
                if anneal_mask & bit:
                    d = F(F(x1) - F(x0))
                    p = F(d * F(progress))
                    h[g, col] = F(F(x0) + p)
        if mode & SCHED_KL:
            hi = F(F(kl_target) * F(kl_factor))
            lo = F(F(kl_target) / F(kl_factor))
            if h[g, KL_COUNT] > 0 and active[g] != 0:
                kl = F(h[g, KL_SUM] / h[g, KL_COUNT])
                rate = h[g, LR]
                if kl > hi:
                    rate = max(F(rate / F(lr_factor)), F(lr_min))
                elif kl < lo:
                    rate = min(F(rate * F(lr_factor)), F(lr_max))
                h[g, LR] = rate
            h[g, KL_SUM] = h[g, KL_COUNT] = F(0.0)
    return h


def kl_table():
    """(hyper fp32 [8, 8], sched_active fp32 [8]): one agent per branch of the KL rule at the default arguments (hi = 0.016, lo = 0.004)."""
    hi, lo = F(F(0.008) * F(2.0)), F(F(0.008) / F(2.0))
    rows = [  # lr,    KL sum,        count, active
        (1e-4, 0.002, 2.0, 1.0),             # 0: mean KL 0.001 < lo: the learning rate grows
        (1e-4, 0.09, 3.0, 1.0),              # 1: mean KL 0.03 > hi: it shrinks
        (1.2e-6, 0.09, 3.0, 1.0),            # 2: ... and stops at lr_min
        (9e-3, 0.002, 2.0, 1.0),             # 3: grows and stops at lr_max
        (1e-4, F(hi * F(2.0)), 2.0, 1.0),    # 4: mean KL == hi exactly: nothing changes
        (1e-4, F(lo * F(2.0)), 2.0, 1.0),    # 5: mean KL == lo exactly: nothing changes
        (1e-4, 5.0, 0.0, 1.0),               # 6: no minibatch counted (a stale sum): nothing changes
        (1e-4, 0.09, 3.0, 0.0),              # 7: a frozen policy: nothing changes
    ]
    h = np.zeros((8, STRIDE), np.float32)
    for g, (rate, s, n, _) in enumerate(rows):
        h[g, LR], h[g, ENTROPY], h[g, RATIO_CLIP], h[g, KL_SUM], h[g, KL_COUNT] = rate, 0.02 + 0.001 * g, 0.15 + 0.01 * g, s, n
    return h, np.array([r[3] for r in rows], np.float32)


ANNEAL_PAIRS = dict(lr=(3e-4, 3e-5), entropy=(0.02, 0.001), ratio_clip=(0.15, 0.3))
ANNEAL_CASES = [(mask, progress) for mask in (1, 2, 4, 7) for progress in (0.0, 1.0 / 3.0, 1.0)]
# by hand (IEEE doubles rounded to fp32 after every operation, outside NumPy): fp32(1e-4) * 1.5, fp32(1e-4) / 1.5, fp32(1e-6), fp32(1e-2);
# and the anneal of fp32(3e-4) -> fp32(3e-5) at fp32(1 / 3) and at 1, where it does NOT land on fp32(3e-5) = 0x1.f75104p-16
KNOWN_KL = {0: float.fromhex("0x1.3a92a2p-13"), 1: float.fromhex("0x1.179ecap-14"), 2: float.fromhex("0x1.0c6f7ap-20"), 3: float.fromhex("0x1.47ae14p-7")}
KNOWN_ANNEAL_LR = {0.0: float.fromhex("0x1.3a92a4p-12"), 1.0 / 3.0: float.fromhex("0x1.b866e4p-13"), 1.0: float.fromhex("0x1.f751p-16")}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


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
    new = {"cat_ppo_loss_grad_dev", "cat_ppo_adam_step_dev", "cat_ppo_schedule_step"}
    assert new <= declared and declared == set(ln.PPO_SYMBOLS) and all(hasattr(L, s) for s in new)
    assert new <= set(ln.MODULES["cat_ppo"][1]) and ln.MODULES["cat_ppo"][0] == 2 and L.cat_ppo_abi_version() == 2
    assert re.search(r"#define CAT_PPO_ABI_VERSION 2\b", code) and re.search(r"#define CAT_PPO_HYPER_STRIDE 8\b", code) and ln.PPO_HYPER_STRIDE == 8
    value = lambda name: int(re.search(r"\b%s = (\d+)" % name, code).group(1))
    names = ("LR", "ENTROPY", "RATIO_CLIP", "KL_SUM", "KL_COUNT")
    assert [value(f"CAT_PPO_HYPER_{n}") for n in names] == [0, 1, 2, 3, 4] == [getattr(ln, f"HYPER_{n}") for n in names]
    assert (value("CAT_PPO_SCHED_KL"), value("CAT_PPO_SCHED_ANNEAL")) == (1, 2) == (ln.SCHED_KL, ln.SCHED_ANNEAL)
    assert [value(f"CAT_PPO_ANNEAL_{n}") for n in names[:3]] == [1, 2, 4] == [ln.ANNEAL_LR, ln.ANNEAL_ENTROPY, ln.ANNEAL_RATIO_CLIP]
    # the _dev structs are the by-value ones with one more pointer at the end
    for dev, plain, cls, base in (("cat_ppo_loss_dev", "cat_ppo_loss", ln.PpoLossDev, ln.PpoLoss), ("cat_ppo_adam_dev", "cat_ppo_adam", ln.PpoAdamDev, ln.PpoAdam)):
        assert _fields(code, dev) == _fields(code, plain) + ["hyper"] == [f[0] for f in cls._fields_]
        assert [f[1] for f in cls._fields_[:-1]] == [f[1] for f in base._fields_] and cls._fields_[-1][1] is C.c_void_p
        assert C.sizeof(cls) == C.sizeof(base) + 8
    assert _fields(code, "cat_ppo_schedule") == [f[0] for f in ln.PpoSchedule._fields_]
    assert _fields(code, "cat_ppo_schedule") == ["G", "mode", "anneal_mask", "pad", "hyper", "sched_active", "kl_target", "kl_factor", "lr_factor",
                                                 "lr_min", "lr_max", "progress", "lr0", "lr1", "ent0", "ent1", "clip0", "clip1"]
    assert C.sizeof(ln.PpoSchedule) == 16 + 2 * 8 + 12 * 4
    assert re.search(r"#define CAT_ROLLOUT_MAX_AGENTS 8\b", (ROOT / "include" / "cat_rollout.h").read_text()) and ln.SCHED_MAX_AGENTS == 8


def _schedule_args(ln, **over):
    kw = dict(G=3, mode=1, anneal_mask=0, pad=0, hyper=4096, sched_active=4096, kl_target=0.008, kl_factor=2.0, lr_factor=1.5, lr_min=1e-6,
              lr_max=1e-2, progress=0.0)
    kw.update(over)
    return ln.PpoSchedule(**kw)


def test_entries_reject_bad_arguments_before_any_device_call():
    """No device here: a call that got past its checks would fail in the runtime (-2) or worse, not return -1 with a message."""
    from as_cops_and_thieves_amd import _learn_native as ln
    L = ln.lib()
    p = 4096                                     # a non-NULL, 8-byte aligned address that no check dereferences
    err = lambda: L.cat_ppo_last_error().decode()
    for entry in (L.cat_ppo_loss_grad_dev, L.cat_ppo_adam_step_dev, L.cat_ppo_schedule_step):
        assert entry(None, None) == -1 and err()
    # the _dev entries: their by-value twins' checks under their own name, then the block
    assert L.cat_ppo_loss_grad_dev(C.byref(ln.PpoLossDev()), None) == -1 and "cat_ppo_loss_grad_dev: bad dimensions" in err()
    assert L.cat_ppo_loss_grad_dev(C.byref(ln.PpoLossDev(3, 5, 64, 0, p, p, None, p, p, p, 0.0, 0.5, 0.0, 0.0, p, p, p, p)), None) == -1 and "NULL" in err()
    assert L.cat_ppo_loss_grad_dev(C.byref(ln.PpoLossDev(3, 5, 64, 0, p, p, p, p, p, p, 0.0, 0.5, 0.0, 0.0, p, p, p, None)), None) == -1
    assert "cat_ppo_loss_grad_dev: hyper is NULL" in err()
    assert L.cat_ppo_adam_step_dev(C.byref(ln.PpoAdamDev()), None) == -1 and "cat_ppo_adam_step_dev: bad dimensions" in err()
    adam = lambda hyper, ar=p: ln.PpoAdamDev(3, 5, 256, 0, ar, p, p, p, p, p, p, None, p, p, 0.0, 0.9, 0.999, 1e-8, 0.5, 0.015, hyper)
    assert L.cat_ppo_adam_step_dev(C.byref(adam(p, ar=None)), None) == -1 and "NULL" in err()
    assert L.cat_ppo_adam_step_dev(C.byref(adam(None)), None) == -1 and "cat_ppo_adam_step_dev: hyper is NULL" in err()
    # the schedule entry: every rejected argument in turn, each with its own message
    for over, message in (({"hyper": None}, "hyper is NULL"), ({"sched_active": None}, "sched_active is NULL"),
                          ({"lr_factor": 0.99}, "lr_factor"), ({"kl_factor": 0.5}, "kl_factor"), ({"lr_min": 1e-2, "lr_max": 1e-3}, "lr_min"),
                          ({"mode": 0}, "mode"), ({"mode": 4}, "mode"), ({"mode": -1}, "mode"),
                          ({"G": 0}, "G must be"), ({"G": 9}, "G must be"),
                          ({"mode": 2, "progress": 1.5}, "progress"), ({"mode": 2, "progress": -0.25}, "progress"),
                          ({"lr_factor": float("nan")}, "lr_factor"), ({"progress": float("nan")}, "progress")):
        assert L.cat_ppo_schedule_step(C.byref(_schedule_args(ln, **over)), None) == -1, over
        assert err().startswith("cat_ppo_schedule_step: ") and message in err(), (over, err())
    # the binding's own asserts come before the library
    with pytest.raises(AssertionError):
        ln.ppo_schedule_step(torch.zeros(3, 7), torch.ones(3), 1)
    with pytest.raises(AssertionError):
        ln.ppo_schedule_step(torch.zeros(9, 8), torch.ones(9), 1)
    with pytest.raises(AssertionError):
        ln.ppo_schedule_step(torch.zeros(3, 8), torch.ones(3, dtype=torch.float64), 1)


# ---------------------------------------------------------------------------------------------- the CPU restatement
def test_cpu_kl_rule_equals_the_numpy_restatement_and_the_known_answers():
    from as_cops_and_thieves_amd.selfplay import mappo
    h0, active = kl_table()
    want = np_schedule(h0, active, SCHED_KL, **KL_ARGS)
    got = torch.from_numpy(h0.copy())
    mappo.schedule_step(got, torch.from_numpy(active), SCHED_KL, **KL_ARGS)
    assert got.dtype == torch.float32 and np.array_equal(_bits(got.numpy()), _bits(want)), (got, want)
    assert not want[:, KL_SUM].any() and not want[:, KL_COUNT].any()                # the sums are cleared in every row
    assert np.array_equal(_bits(want[:, [ENTROPY, RATIO_CLIP]]), _bits(h0[:, [ENTROPY, RATIO_CLIP]])) and not want[:, 5:].any()
    for g, answer in KNOWN_KL.items():
        assert float(want[g, LR]) == answer, (g, float(want[g, LR]).hex())
    assert want[0, LR] > h0[0, LR] and want[1, LR] < h0[1, LR] and want[2, LR] == F(1e-6) and want[3, LR] == F(1e-2)
    assert np.array_equal(_bits(want[4:, LR]), _bits(h0[4:, LR]))                   # kl == hi, kl == lo, no count, frozen: unchanged
    # one ulp beyond the band's edges the rule does move the rate: the edges themselves are compared strictly
    edge = h0.copy()
    edge[4, KL_SUM], edge[5, KL_SUM] = np.nextafter(h0[4, KL_SUM], F(1)), np.nextafter(h0[5, KL_SUM], F(0))
    moved = np_schedule(edge, active, SCHED_KL, **KL_ARGS)
    assert moved[4, LR] == want[1, LR] and moved[5, LR] == want[0, LR]
    got = torch.from_numpy(edge.copy())
    mappo.schedule_step(got, torch.from_numpy(active), SCHED_KL, **KL_ARGS)
    assert np.array_equal(_bits(got.numpy()), _bits(moved))


@pytest.mark.parametrize("mask,progress", ANNEAL_CASES)
def test_cpu_anneal_equals_the_numpy_restatement_and_the_known_answers(mask, progress):
    from as_cops_and_thieves_amd.selfplay import mappo
    h0, active = kl_table()
    active[:] = 0.0                             # the anneal reaches every agent, frozen or not
    for mode in (SCHED_ANNEAL, SCHED_ANNEAL | SCHED_KL):
        want = np_schedule(h0, active, mode, anneal_mask=mask, progress=progress, **ANNEAL_PAIRS, **KL_ARGS)
        got = torch.from_numpy(h0.copy())
        mappo.schedule_step(got, torch.from_numpy(active), mode, anneal_mask=mask, progress=progress, **ANNEAL_PAIRS, **KL_ARGS)
        assert np.array_equal(_bits(got.numpy()), _bits(want)), (mode, got, want)
        for bit, col in ((1, LR), (2, ENTROPY), (4, RATIO_CLIP)):
            if not mask & bit:
                assert np.array_equal(_bits(want[:, col]), _bits(h0[:, col]))
            else:
                assert len(set(want[:, col].tolist())) == 1
        if mask & 1:
            assert float(want[0, LR]) == KNOWN_ANNEAL_LR[progress], float(want[0, LR]).hex()
        sums = want[:, [KL_SUM, KL_COUNT]]
        assert not sums.any() if mode & SCHED_KL else np.array_equal(_bits(sums), _bits(h0[:, [KL_SUM, KL_COUNT]]))


def test_the_restatement_rejects_what_the_entry_rejects():
    from as_cops_and_thieves_amd.selfplay import mappo
    h, active = torch.zeros(2, 8), torch.ones(2)
    for kw in ({"lr_factor": 0.5}, {"kl_factor": 0.5}, {"lr_min": 1.0, "lr_max": 0.5}, {"progress": 1.5}):
        with pytest.raises(ValueError):
            mappo.schedule_step(h, active, SCHED_KL, **kw)
    for mode in (0, 4):
        with pytest.raises(ValueError):
            mappo.schedule_step(h, active, mode)


# ---------------------------------------------------------------------------------------------- the learner on the CPU
EPOCHS, UPDATES, LEARNING_RATE = 2, 2, 3e-3


def _env(n=6, seed=1):
    from as_cops_and_thieves_amd.maps import load_preset
    from tests.fake_env import OracleVecEnv
    return OracleVecEnv(load_preset("squarinth").compile(), n, num_rays=16, max_step_count=12, seed=seed)


def _trainer(seed=0, **rc_kw):
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
    rc = RoleConfig(learning_epochs=EPOCHS, mini_batches=2, random_timesteps=0, learning_starts=0, learning_rate=LEARNING_RATE, **rc_kw)
    tc = TrainerConfig(horizon=4, policy_freeze_duration=0, opponent_freeze_duration=0)
    return MAPPOTrainer(_env(), {"cop": rc, "thief": rc}, tc, seed=seed)


def _run(tr, updates=UPDATES):
    for _ in range(updates):
        tr.collect(); tr.update()
    return tr.param_digest()


def _shrunk(steps, **kw):
    """fp32(LEARNING_RATE) after ``steps`` shrink steps of the KL rule, by the restatement above"""
    h = np.zeros((1, STRIDE), np.float32)
    h[0, LR] = LEARNING_RATE
    for _ in range(steps):
        h[0, KL_SUM], h[0, KL_COUNT] = 1.0, 1.0
        h = np_schedule(h, np.ones(1, np.float32), SCHED_KL, **dict(KL_ARGS, kl_target=1e-12, **kw))
    return float(h[0, LR])


@pytest.fixture(scope="module")
def plain_digest():
    tr = _trainer()
    (rl,) = tr.roles.values()
    assert not rl.scheduled and not hasattr(rl, "hyper") and not hasattr(rl, "sched_active")
    digest = _run(tr)
    assert not any(k.startswith(("lr/", "entropy_scale/", "ratio_clip/")) for k in tr.read_stats())
    assert "schedule" not in tr.state_dict()[tr.agents[0]]
    return digest


def test_schedules_that_change_nothing_train_as_the_unscheduled_trainer(plain_digest):
    twins = ({"lr_schedule": "kl_adaptive", "lr_factor": 1.0},
             {"lr_schedule": "linear", "lr_final": LEARNING_RATE, "entropy_final": 0.02, "ratio_clip_final": 0.15, "schedule_updates": 3})
    for kw in twins:
        tr = _trainer(**kw)
        (rl,) = tr.roles.values()
        assert rl.scheduled and rl.hyper.shape == (rl.G, 8) and rl.hyper.dtype == torch.float32 and rl.sched_active.tolist() == [1.0] * rl.G
        assert _run(tr) == plain_digest, kw
        stats = tr.read_stats()
        for a in tr.agents:
            assert (stats[f"lr/{a}"], stats[f"entropy_scale/{a}"], stats[f"ratio_clip/{a}"]) == (float(F(LEARNING_RATE)), float(F(0.02)), float(F(0.15)))
        assert not rl.hyper[:, 3:].any() or kw["lr_schedule"] == "linear"          # the KL rule leaves empty sums behind
        assert rl.updates_done == UPDATES


def test_a_tiny_kl_target_shrinks_the_rate_every_epoch(plain_digest):
    tr = _trainer(lr_schedule="kl_adaptive", lr_kl_target=1e-12)
    digest = _run(tr)
    stats = tr.read_stats()
    want = _shrunk(EPOCHS * UPDATES)
    assert want < LEARNING_RATE / 5 and [stats[f"lr/{a}"] for a in tr.agents] == [want] * len(tr.agents)
    assert digest != plain_digest
    sd = tr.state_dict()
    for a in tr.agents:         # the checkpoint's Adam entry reports the agent's current learning rate
        assert sd[a]["optimizer"]["param_groups"][0]["lr"] == want and sd[a]["schedule"]["lr"] == want


def test_a_huge_kl_target_grows_the_rate_to_lr_max():
    tr = _trainer(lr_schedule="kl_adaptive", lr_kl_target=1e3)
    _run(tr)
    stats = tr.read_stats()
    assert [stats[f"lr/{a}"] for a in tr.agents] == [float(F(1e-2))] * len(tr.agents)      # 3e-3 * 1.5^4 > lr_max


def test_a_frozen_policy_keeps_its_learning_rate():
    tr = _trainer(lr_schedule="kl_adaptive", lr_kl_target=1e3)
    (rl,) = tr.roles.values()
    tr.set_frozen(role="thief", policy=True)
    assert rl.sched_active.tolist() == [0.0 if r == "thief" else 1.0 for r in rl.agent_roles] and rl.rows("thief") and rl.rows("cop")
    _run(tr)
    stats = tr.read_stats()
    for a in tr.agents:
        assert stats[f"lr/{a}"] == (float(F(LEARNING_RATE)) if a.startswith("thief") else float(F(1e-2))), a
    assert not rl.hyper[:, 3:].any()
    tr.set_frozen(role="thief", policy=False)
    assert rl.sched_active.tolist() == [1.0] * rl.G


def test_linear_anneals_follow_the_updates_and_stop_at_the_end():
    kw = dict(lr_schedule="linear", lr_final=3e-4, entropy_final=0.001, ratio_clip_final=0.3, schedule_updates=3)
    tr = _trainer(**kw)
    (rl,) = tr.roles.values()
    pairs = dict(lr=(LEARNING_RATE, 3e-4), entropy=(0.02, 0.001), ratio_clip=(0.15, 0.3))
    for k in range(5):          # update k trains at progress min(1, k / 3)
        tr.collect(); tr.update()
        want = np_schedule(np.zeros((1, STRIDE), np.float32), np.ones(1, np.float32), SCHED_ANNEAL, anneal_mask=7, progress=min(1.0, k / 3), **pairs)
        assert np.array_equal(_bits(rl.hyper[:, :3].numpy()), _bits(np.repeat(want[:, :3], rl.G, 0))), k
        assert not rl.hyper[:, 5:].any()
    assert rl.updates_done == 5


# ---------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_round_trip_and_a_trainer_without_schedules():
    """An uninterrupted run of three updates against one that is saved after the first, loaded and continued.  The checkpoint holds no env:
    the second trainer plays the same first rollout and update (same seeds: same env, generator and recurrent states as the first at the time
    of saving), then everything the checkpoint should restore is spoilt -- parameters, Adam, the hyper block, the anneals' clock -- and loaded.
    Both start with ``set_frozen(policy=False, value=False)``, as ``train()`` does: the trainable columns are then the named parameters alone,
    and the step counts of the flat buffer's padding, which no checkpoint carries, stay 0 in both."""
    kw = dict(lr_schedule="kl_adaptive", lr_kl_target=1e-12, entropy_final=0.001, schedule_updates=3)
    a = _trainer(**kw)
    a.set_frozen(policy=False, value=False)
    _run(a, 1)
    sd = a.state_dict()
    digest = _run(a, 2)
    for ag in a.agents:
        assert set(sd[ag]["schedule"]) == {"lr", "entropy_scale", "ratio_clip", "updates"} and sd[ag]["schedule"]["updates"] == 1
        assert sd[ag]["schedule"]["lr"] == _shrunk(EPOCHS) == sd[ag]["optimizer"]["param_groups"][0]["lr"]
    b = _trainer(**kw)
    b.set_frozen(policy=False, value=False)
    _run(b, 1)
    (rl,) = b.roles.values()
    for t, by in ((rl.fp.master, 0.25), (rl.m, 1.0), (rl.v, 1.0), (rl.steps, 3.0)):          # (the named parameters: not the padding)
        t.add_(by * rl.col_train)
    rl.fp.refresh()
    rl.hyper.fill_(0.5); rl.updates_done = 17
    b.load_state_dict(sd)
    assert rl.updates_done == 1 and not rl.hyper[:, 3:].any()
    assert _run(b, 2) == digest
    sa, sb = a.read_stats(), b.read_stats()
    for ag in a.agents:
        for k in (f"lr/{ag}", f"entropy_scale/{ag}", f"ratio_clip/{ag}"):
            assert sa[k] == sb[k], k
        assert sa[f"lr/{ag}"] == _shrunk(3 * EPOCHS)
    # an entry without the values starts from the config
    old = {ag: {k: v for k, v in e.items() if k != "schedule"} if ag in a.agents else e for ag, e in sd.items()}
    b.load_state_dict(old)
    assert rl.updates_done == 0 and rl.hyper[:, :3].tolist() == [[float(F(LEARNING_RATE)), float(F(0.02)), float(F(0.15))]] * rl.G
    # a copy of the models alone (the self-play loop's start of an iteration) leaves the schedule as it is
    rl.updates_done = 2
    b.load_state_dict(sd, optimizer=False)
    assert rl.updates_done == 2
    # ... and a trainer without schedules ignores the values with ONE warning
    c = _trainer()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        c.load_state_dict(sd)
    assert len([w for w in caught if "schedule" in str(w.message)]) == 1
    assert not hasattr(next(iter(c.roles.values())), "hyper") and "schedule" not in c.state_dict()[c.agents[0]]


# ---------------------------------------------------------------------------------------------- configuration
def test_defaults_are_off_and_bad_configurations_name_their_field():
    from as_cops_and_thieves_amd.selfplay import mappo
    rc = mappo.RoleConfig()
    assert dataclasses.is_dataclass(rc) and not mappo.scheduled(rc)
    assert (rc.lr_schedule, rc.lr_final, rc.entropy_final, rc.ratio_clip_final, rc.schedule_updates) == ("constant", None, None, None, 0)
    assert (rc.lr_kl_target, rc.lr_kl_factor, rc.lr_factor, rc.lr_min, rc.lr_max) == (0.008, 2.0, 1.5, 1e-6, 1e-2)
    assert rc.kl_threshold == 0.015                                              # the early-stop gate is another number
    assert not any(mappo.scheduled(c) for c in (mappo.CFG_AGENT, mappo.CFG_AGENT_COP, mappo.CFG_AGENT_THIEF))
    for kw, field in (({"lr_schedule": "cosine"}, "lr_schedule"), ({"lr_schedule": "linear", "schedule_updates": 4}, "lr_final"),
                      ({"lr_schedule": "linear", "lr_final": 1e-5}, "schedule_updates"), ({"entropy_final": 0.0}, "schedule_updates"),
                      ({"ratio_clip_final": 0.1, "schedule_updates": -2}, "schedule_updates"),
                      ({"lr_schedule": "kl_adaptive", "lr_factor": 0.5}, "lr_factor"), ({"lr_schedule": "kl_adaptive", "lr_kl_factor": 0.5}, "lr_kl_factor"),
                      ({"lr_schedule": "kl_adaptive", "lr_min": 1.0}, "lr_min")):
        with pytest.raises(ValueError, match=field):
            _trainer(**kw)
    # roles configured alike still stack into one learner, scheduled or not
    assert list(_trainer(lr_schedule="kl_adaptive").roles) == ["cop+thief"]


def test_run_self_play_plans_the_anneals_over_its_updates():
    from as_cops_and_thieves_amd.selfplay.mappo import RoleConfig, TrainerConfig
    from as_cops_and_thieves_amd.selfplay.self_play import planned_updates
    tc = TrainerConfig(timesteps=100, horizon=16)
    assert planned_updates(1, tc, RoleConfig(learning_starts=0)) == 7                # rollouts end at 16, 32, .., 112
    assert planned_updates(3, tc, RoleConfig(learning_starts=40)) == 3 * 5            # the first update follows the rollout that ends at 48
    assert planned_updates(2, tc, RoleConfig(learning_starts=10_000)) == 1


def test_run_self_play_passes_the_schedule_into_both_roles_and_logs_the_rates(tmp_path):
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import RoleConfig, TrainerConfig
    from as_cops_and_thieves_amd.selfplay.self_play import TrainingConfig, run_self_play
    from tests.fake_env import OracleVecEnv
    cmap = load_preset("squarinth").compile()
    rc = RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=4, learning_starts=8, kl_threshold=0.0, learning_rate=LEARNING_RATE)
    lines = []
    run_self_play("squarinth", 8, tmp_path, iterations=2, training=TrainingConfig(n_trial_episodes=2, num_opponents_to_evaluate=1),
                  trainer_cfg=TrainerConfig(horizon=4, timesteps=16, policy_freeze_duration=8, opponent_freeze_duration=8),
                  role_cfg={"cop": rc, "thief": rc}, env_factory=lambda n, s: OracleVecEnv(cmap, n, num_rays=16, max_step_count=12, seed=s),
                  log=lambda *a: lines.append(" ".join(map(str, a))), lr_schedule="linear", lr_final=3e-4, entropy_final=0.001)
    sd = torch.load(tmp_path / "joint_iter_1_full_agent.pt", weights_only=True)
    # 4 rollouts per iteration, the first update after the one that ends at learning_starts = 8: 3 updates x 2 iterations, planned as 6
    want = np_schedule(np.zeros((1, STRIDE), np.float32), np.ones(1, np.float32), SCHED_ANNEAL, anneal_mask=3, progress=5 / 6,
                       lr=(LEARNING_RATE, 3e-4), entropy=(0.02, 0.001))
    for a in ("cop_0", "cop_1", "thief_0"):
        assert sd[a]["schedule"] == {"lr": float(want[0, LR]), "entropy_scale": float(want[0, ENTROPY]), "ratio_clip": float(F(0.15)), "updates": 6}
    saved = [ln for ln in lines if "saved joint_iter_" in ln]
    assert len(saved) == 2 and all("; lr cop_0=" in ln for ln in saved)
