"""What the eight modules of libcat_learn.so share (csrc/cat_learn_common.h, the binding's ``MODULES`` table and its one bounds check), as
far as a host without a device can see it: the argument checks of every entry run before any device call."""
import ctypes as C
import os
import types

import pytest

from as_cops_and_thieves_amd import _learn_native as ln


def _bad_calls(L):
    """module -> two calls that fail their argument checks with DIFFERENT messages"""
    z = lambda cls: C.byref(cls())
    return {
        "cat_lstm": (lambda: L.cat_lstm_seq_forward(z(ln.FwdArgs), None), lambda: L.cat_lstm_seq_backward(z(ln.BwdArgs), None)),
        "cat_trunk": (lambda: L.cat_trunk_forward(z(ln.TrunkFwd), None), lambda: L.cat_trunk_backward(z(ln.TrunkBwd), None)),
        "cat_ppo": (lambda: L.cat_ppo_loss_grad(z(ln.PpoLoss), None), lambda: L.cat_ppo_adam_step(z(ln.PpoAdam), None)),
        "cat_dense": (lambda: L.cat_dense_bias_act(C.byref(ln.DenseDims(1, 1, 3, 0)), None, None, 0, None), lambda: L.cat_dense_wgrad(z(ln.WgradArgs), None)),
        "cat_rollout": (lambda: L.cat_rollout_pack(z(ln.PackArgs), None), lambda: L.cat_rollout_sample(z(ln.SampleArgs), None)),
        "cat_render": (lambda: L.cat_render_frames(None, None, None), lambda: L.cat_render_frames(z(ln.RenderSceneDesc), z(ln.RenderArgs), None)),
        "cat_episodes": (lambda: L.cat_episodes_update(z(ln.EpisodesUpdate), None), lambda: L.cat_episodes_summary(z(ln.EpisodesSummary), None)),
        "cat_act": (lambda: L.cat_act_step(z(ln.ActArgs), None), lambda: L.cat_act_league_step(z(ln.ActLeagueArgs), None)),
    }


def test_a_bad_argument_sets_only_its_own_modules_error():
    ln.build()
    L = ln.lib()
    calls = _bad_calls(L)
    assert set(calls) == set(ln.MODULES)
    errors = lambda: {m: getattr(L, f"{m}_last_error")() for m in ln.MODULES}
    for first, _ in calls.values():                     # every module holds a message of its own
        assert first() == -1
    held = errors()
    assert all(held.values()) and len(set(held.values())) == len(held)
    for module, (_, second) in calls.items():
        assert second() == -1, module
        now = errors()
        assert now[module] and now[module] != held[module], module
        assert {m: e for m, e in now.items() if m != module} == {m: e for m, e in held.items() if m != module}, module
        held = now


def test_every_table_symbol_resolves_and_abi_versions_match():
    ln.build()
    L = ln.lib()
    for module, (abi, entries) in ln.MODULES.items():
        for sym in (f"{module}_abi_version", f"{module}_last_error", *entries):
            assert hasattr(L, sym), sym
        assert getattr(L, f"{module}_abi_version")() == abi, module
    by_tuple = (ln.EXPORTED_SYMBOLS + ln.TRUNK_SYMBOLS + ln.PPO_SYMBOLS + ln.DENSE_SYMBOLS + ln.ROLLOUT_SYMBOLS + ln.RENDER_SYMBOLS +
                ln.EPISODES_SYMBOLS + ln.EPISODE_WINDOWS_SYMBOLS + ln.EPISODE_SEGMENTS_SYMBOLS + ln.ACT_SYMBOLS)
    in_table = [s for m, (_, entries) in ln.MODULES.items() for s in (f"{m}_abi_version", f"{m}_last_error", *entries)]
    assert sorted(by_tuple) == sorted(in_table) and len(set(in_table)) == len(in_table)


@pytest.mark.parametrize("N,bounds", [(8, [0]), (33, list(range(34))), (8, [1, 8]), (8, [0, 7]), (8, [0, 4, 4, 8])],
                         ids=["0 segments", "33 segments", "first not 0", "last not N", "repeated bound"])
def test_the_shared_bounds_check_rejects_before_the_library_is_touched(monkeypatch, N, bounds):
    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(ln, "lib", touched)
    S = len(bounds) - 1
    with pytest.raises(ValueError) as e1:
        ln.segment_bounds(N, bounds)
    with pytest.raises(ValueError) as e2:
        ln.league_table(N, 2, 1, bounds, [[0] * S] * 2)
    assert str(e1.value) == str(e2.value)               # one rule, one message (ACT_MAX_SEGMENTS == EPISODES_MAX_SEGMENTS)
    assert ln.segment_bounds(8, [0, 3, 8]) == [0, 3, 8] and ln.league_table(8, 2, 1, [0, 3, 8], [[0, -1]] * 2).start == [0, 3, 8]


def test_the_internal_header_is_an_input_of_the_build(monkeypatch, tmp_path):
    header = ln.PKG / "csrc" / "cat_learn_common.h"
    assert header in ln.INTERNAL_HEADERS and header.exists() and header not in ln.HEADERS and not header.name.startswith("cat_sim_")
    assert all('#include "cat_learn_common.h"' in src.read_text() for src in ln.SOURCES)
    # build() compiles again exactly when an internal header is newer than the library
    lib, hdr, runs = tmp_path / "lib.so", tmp_path / "internal.h", []
    lib.write_bytes(b"")
    hdr.write_text("")
    newest = max(f.stat().st_mtime for f in ln.SOURCES + ln.HEADERS)
    os.utime(lib, (newest + 10, newest + 10))
    monkeypatch.setattr(ln, "LIB_PATH", lib)
    monkeypatch.setattr(ln, "INTERNAL_HEADERS", (hdr,))
    monkeypatch.setattr(ln.subprocess, "run", lambda cmd, **kw: runs.append(cmd) or types.SimpleNamespace(returncode=0, stdout="", stderr=""))
    os.utime(hdr, (newest + 5, newest + 5))
    ln.build()
    assert runs == []
    os.utime(hdr, (newest + 20, newest + 20))
    ln.build()
    assert len(runs) == 1 and str(ln.SOURCES[0]) in runs[0]
