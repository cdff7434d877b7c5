"""CPU: the collect form of the act tick -- ``cat_act_collect_args`` in include/cat_act.h against the library and its ctypes mirror, the entry's
argument checks (no device needed) -- and ``TrainerConfig.fused_collect`` as far as a host without a device sees it."""
import ctypes as C
import re
import warnings
from pathlib import Path

import pytest
import torch

from as_cops_and_thieves_amd import _learn_native as ln
from as_cops_and_thieves_amd.maps import load_preset
from as_cops_and_thieves_amd.selfplay import mappo
from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
from tests.fake_env import OracleVecEnv

warnings.filterwarnings("ignore", message="grad and param do not obey the gradient layout contract")
ROOT = Path(__file__).resolve().parents[1]
CMAP = load_preset("squarinth", 2, 1).compile()
RC = RoleConfig(learning_epochs=1, mini_batches=2, random_timesteps=4, learning_starts=8, kl_threshold=0.0)


# ---------------------------------------------------------------------------------------------- 1. header, library, mirror
def test_collect_header_matches_the_library_and_the_ctypes_mirror():
    from tests.test_abi_and_isolation import test_learner_kernel_headers_match_the_library_and_the_ctypes_mirror as header_check
    header_check("cat_act.h", "cat_act_", "ACT_SYMBOLS", {"cat_act_dims": "ActDims", "cat_act_params": "ActParams", "cat_act_args": "ActArgs",
                                                         "cat_act_collect_args": "ActCollectArgs", "cat_act_league_args": "ActLeagueArgs"})
    L = ln.lib()
    assert hasattr(L, "cat_act_collect_step") and ln.ACT_SYMBOLS[-1] == "cat_act_league_step"
    assert ln.ACT_SYMBOLS.index("cat_act_step") + 1 == ln.ACT_SYMBOLS.index("cat_act_collect_step") == len(ln.ACT_SYMBOLS) - 2
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_act.h").read_text(), flags=re.S)
    assert int(re.search(r"#define CAT_ACT_ABI_VERSION (\d+)", code).group(1)) == 1 == L.cat_act_abi_version()
    protos = re.findall(r"\bint (cat_act_[a-z_]*step)\(", code)
    assert protos == ["cat_act_step", "cat_act_collect_step", "cat_act_league_step"]
    # the older structs keep their sizes; the new one: base, two ints, then fourteen 8-byte members
    assert C.sizeof(ln.ActArgs) == 280 and C.sizeof(ln.ActLeagueArgs) == 1448
    assert C.sizeof(ln.ActCollectArgs) == 280 + 2 * 4 + 14 * 8 == 400 < 4096
    assert (ln.ActCollectArgs.base.offset, ln.ActCollectArgs.n_cops.offset, ln.ActCollectArgs.shared_distance.offset) == (0, 280, 288)
    assert ln.ActCollectArgs.c0_out.offset + 8 == C.sizeof(ln.ActCollectArgs)
    assert ln.SOURCES[-1].name == "cat_act.hip" and len(ln.SOURCES) == 8


# ---------------------------------------------------------------------------------------------- 2. the entry's argument checks
FAKE = 0x100000        # a 16-byte aligned address that is never dereferenced: every call below fails a check before any device call


def _collect_args(R=64, N=10):
    a = ln.ActCollectArgs()
    a.base.d = ln.ActDims(3, N, 3, R)
    for g in range(3):
        a.base.agent[g] = g
    for name in ("obs_distance", "obs_type", "h", "c", "uniform", "actions"):
        setattr(a.base, name, FAKE)
    for name in ln.ACT_PARAM_FIELDS:
        setattr(a.base.p, name, FAKE)
    a.base.p.stride = 8
    a.n_cops = 2
    for name in ("shared_distance", "shared_type", "policy_in", "value_in", "act_out", "logp_out", "h0_out", "c0_out"):
        setattr(a, name, FAKE)
    a.sp_g, a.sp_n, a.sv_g, a.sv_n, a.sa_g, a.sl_g = 3 * N * 2 * R, 2 * R, 3 * N * 4 * R, 4 * R, 3 * N, 3 * N
    return a


def _rejected(a, word):
    L = ln.lib()
    rc, msg = L.cat_act_collect_step(C.byref(a), None), L.cat_act_last_error()
    assert rc == -1 and word in msg and msg.startswith(b"cat_act_collect_step:"), (rc, msg, word)
    return msg


def test_collect_entry_rejects_each_class_of_bad_argument_before_touching_a_device():
    L = ln.lib()
    assert L.cat_act_collect_step(None, None) == -1
    seen = set()
    for dims in ((3, 10, 3, 72), (9, 10, 3, 64), (3, 0, 3, 64)):
        a = _collect_args()
        a.base.d = ln.ActDims(*dims)
        seen.add(_rejected(a, b"dimensions"))
    for name in ("shared_distance", "shared_type", "policy_in", "value_in", "act_out", "logp_out"):     # NULLs of the collect form
        a = _collect_args()
        setattr(a, name, None)
        seen.add(_rejected(a, b"collect buffer is NULL"))
    for name in ("obs_distance", "uniform", "actions"):                                                # NULLs of the base
        a = _collect_args()
        setattr(a.base, name, None)
        seen.add(_rejected(a, b"NULL"))
    a = _collect_args()
    a.base.h = None
    seen.add(_rejected(a, b"NULL"))
    for mask in (1, 0b100):                                                                            # a learner never acts at random
        a = _collect_args()
        a.base.random_mask = mask
        seen.add(_rejected(a, b"random_mask must be 0"))
    for name, off in (("policy_in", 4), ("value_in", 2), ("act_out", 4), ("logp_out", 2), ("h0_out", 8), ("c0_out", 8)):   # misaligned pointers
        a = _collect_args()
        setattr(a, name, FAKE + off)
        seen.add(_rejected(a, b"misaligned"))
    for R in (64, 90):                                                                                 # misaligned or short strides
        for name, v in (("sp_g", 2 * R * 30 + 2), ("sp_n", 2 * R + 2), ("sv_g", 4 * R * 30 + 1), ("sv_n", 4 * R + 3), ("sp_n", 2 * R - 4), ("sv_n", 4 * R - 4)):
            a = _collect_args(R)
            setattr(a, name, v)
            seen.add(_rejected(a, b"stride"))
    for name in ("h0_out", "c0_out"):                                                                  # one of the pair alone
        a = _collect_args()
        setattr(a, name, None)
        seen.add(_rejected(a, b"together"))
    a = _collect_args()
    a.n_cops = 4
    seen.add(_rejected(a, b"n_cops"))
    assert len(seen) >= 8                                                                              # every class has a message of its own
    # the other entries keep their messages
    assert L.cat_act_step(C.byref(ln.ActArgs()), None) == -1 and L.cat_act_last_error().startswith(b"cat_act_step: bad dimensions")


# ---------------------------------------------------------------------------------------------- 3. the trainer option
def test_fused_collect_on_the_cpu_raises_and_names_what_is_missing():
    env = OracleVecEnv(CMAP, 8, num_rays=16, max_step_count=12, seed=3)
    with pytest.raises(ValueError) as e:
        MAPPOTrainer(env, {"cop": RC, "thief": RC}, TrainerConfig(horizon=4, fused_collect=True), seed=2)
    msg = str(e.value)
    assert "fused_collect" in msg and "a GPU" in msg and "raw_outputs" in msg and "64 or 90 rays" in msg
    assert "bf16" not in msg and "recurrent" not in msg and "deferred_values" not in msg and "random_action_roles" not in msg
    for kw, word in ((dict(compute_bf16=False), "bf16"), (dict(recurrent=False), "recurrent"), (dict(deferred_values=False), "deferred_values"),
                     (dict(random_action_roles=("thief",)), "random_action_roles")):
        with pytest.raises(ValueError) as e:
            MAPPOTrainer(env, {"cop": RC, "thief": RC}, TrainerConfig(horizon=4, fused_collect=True, **kw), seed=2)
        assert word in str(e.value) and "a GPU" in str(e.value), (word, str(e.value))


def test_without_the_option_the_rollout_makes_todays_calls(monkeypatch):
    assert TrainerConfig().fused_collect is False

    def forbidden(*a, **k):
        raise AssertionError("the collect tick ran without fused_collect")
    monkeypatch.setattr(ln, "act_collect_step", forbidden)
    monkeypatch.setattr(MAPPOTrainer, "_collect_tick", forbidden)
    runs = []
    for tcfg in (TrainerConfig(horizon=4, bptt=4), TrainerConfig(horizon=4, bptt=4, fused_collect=False)):
        env = OracleVecEnv(CMAP, 8, num_rays=16, max_step_count=12, seed=3)
        runner = MAPPOTrainer(env, {"cop": RC, "thief": RC}, tcfg, seed=2)
        calls = []
        for rl in runner.roles.values():
            for net, fwd in (("policy", rl.policy.forward), ("value", rl.value.forward)):
                setattr(getattr(rl, net), "forward", lambda *a, _f=fwd, _n=net, **k: (calls.append(_n), _f(*a, **k))[1])
        torch.manual_seed(9)
        runner.collect()
        (rl,) = runner.roles.values()
        runs.append((calls, {k: v.clone() for k, v in rl.buf.items()}))
    assert runs[0][0] == ["policy", "value"] * 4 == runs[1][0]              # per tick the policy chain, then the critic: today's CPU rollout
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
    assert mappo._learn_native is ln
