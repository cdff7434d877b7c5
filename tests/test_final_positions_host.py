"""End-of-episode positions without a GPU: the new env-core entry is exported, declared and bound; ``CatSim.bind_final_positions`` refuses a
wrong buffer before any native call; the NumPy form of the capture / timeout maps (``positions.PositionTracker(final_positions=True)``) on
hand-made rows with every integer written out; the C ABI of ``cat_render_positions_ends_update`` and its argument checks; the two new
heatmap files; and a tracker without final positions gives what it gave before, key for key."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from as_cops_and_thieves_amd.maps import PLANE_STRIDE, CompiledMap
from as_cops_and_thieves_amd.positions import PositionTracker

ROOT = Path(__file__).resolve().parents[1]
NAN = float("nan")
SENTINEL = 0x7E00


# ---------------------------------------------------------------------------------------------- 1. the env-core entry and its binding
def test_bind_final_positions_is_exported_declared_and_bound():
    from as_cops_and_thieves_amd import _native as nat
    from as_cops_and_thieves_amd import sim
    assert "cat_bind_final_positions" in nat.EXPORTED_SYMBOLS
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_sim.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+cat_bind_final_positions\s*\(\s*cat_sim\s*\*\s*sim\s*,\s*uint16_t\s*\*\s*buf\s*\)\s*;", header)
    assert re.search(r"#define CAT_ABI_VERSION 1\b", header)                    # an entry added to version 1, no new field of cat_outputs
    assert "final" not in re.search(r"typedef struct cat_outputs \{(.*?)\} cat_outputs;", header, re.S).group(1)
    nat.build()
    L = nat.lib()
    assert L.cat_abi_version() == 1
    assert L.cat_bind_final_positions.argtypes == [C.c_void_p, C.c_void_p]
    assert L.cat_bind_final_positions(None, None) == -6                        # CAT_ERR_BAD_ARG: no handle
    assert sim.FINAL_POS_NAN == SENTINEL and np.isnan(np.array([SENTINEL], np.uint16).view(np.float16)[0])


class _NoNativeCall:
    def __getattr__(self, name):
        raise AssertionError(f"native entry {name} was reached")


def test_bind_final_positions_refuses_a_wrong_buffer_before_any_native_call():
    from as_cops_and_thieves_amd.sim import CatSim
    sim = CatSim.__new__(CatSim)                                # no device here: the checks need none
    sim._h, sim._L, sim.N, sim.A, sim.device = None, _NoNativeCall(), 5, 3, torch.device("cuda", 0)
    good = torch.zeros(5, 3, 2, dtype=torch.float16)           # right in everything but the device
    bad = {"dtype": torch.zeros(5, 3, 2, dtype=torch.float32), "dtype (the raw bits)": torch.zeros(5, 3, 2, dtype=torch.int16),
           "shape": torch.zeros(5, 2, 2, dtype=torch.float16), "flat": torch.zeros(30, dtype=torch.float16),
           "[T, N, A, 2] of another N": torch.zeros(4, 6, 3, 2, dtype=torch.float16), "T = 0": torch.zeros(0, 5, 3, 2, dtype=torch.float16),
           "device": good, "device, [T, N, A, 2]": torch.zeros(7, 5, 3, 2, dtype=torch.float16), "no tensor": np.zeros((5, 3, 2), np.float16)}
    for what, buf in bad.items():
        with pytest.raises(ValueError, match="final positions"):
            sim.bind_final_positions(buf)
        assert not hasattr(sim, "_final_pos"), what
    # the checks by themselves, against the device the buffers do lie on: both layouts pass, a strided view does not
    CatSim.check_final_positions(good, 5, 3, "cpu")
    CatSim.check_final_positions(torch.zeros(7, 5, 3, 2, dtype=torch.float16), 5, 3, "cpu")
    with pytest.raises(ValueError, match="contiguous"):
        CatSim.check_final_positions(torch.zeros(5, 3, 4, dtype=torch.float16)[:, :, ::2], 5, 3, "cpu")
    with pytest.raises(ValueError, match="device|live on"):
        CatSim.check_final_positions(good, 5, 3, "cuda:0")


# ---------------------------------------------------------------------------------------------- 2. the NumPy form of the ends update
def _hand_made():
    """T = 3, N = 4, A = 3, window 96 x 64, cell 32 (3 x 2 cells), groups (0, 1, -1, 0), quota (5, 5, 5, 1)."""
    T, N, A = 3, 4, 3
    final = np.full((T, N, A, 2), SENTINEL, np.uint16).view(np.float16)
    team = np.zeros((T, N, A, 2), np.float16)                   # the spawn / occupancy positions: all in cell (0, 0)
    team[...] = 1.0
    term, trunc = np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint8)
    term[0, 0] = 1                                              # slot 0, row 0: a capture; agent 2 has a NaN coordinate
    final[0, 0] = [(10.0, 10.0), (40.0, 40.0), (NAN, 5.0)]
    term[2, 0] = trunc[2, 0] = 1                                # slot 0, row 2: a timeout; agent 1 has a negative coordinate
    final[2, 0] = [(70.0, 5.0), (-1.0, 5.0), (5.0, 40.0)]
    final[0, 1] = [(10.0, 10.0)] * 3                            # slot 1, row 0: NOT terminal -- a valid position that must not be read
    term[1, 1] = trunc[1, 1] = 1                                # slot 1 (group 1), row 1: a timeout; agent 1 lies off the grid
    final[1, 1] = [(95.0, 63.0), (200.0, 10.0), (33.0, 0.0)]
    term[1, 2] = 1                                              # slot 2: group -1, never counted
    final[1, 2] = [(50.0, 50.0)] * 3
    term[1, 3] = 1                                              # slot 3 (group 0, quota 1), row 1: a capture ...
    final[1, 3] = [(64.0, 32.0), (0.0, 0.0), (31.9, 31.9)]
    term[2, 3] = trunc[2, 3] = 1                                # ... and row 2 a second terminal row: skipped by the quota
    final[2, 3] = [(50.0, 50.0)] * 3
    return final, team, term, trunc, np.array([0, 1, -1, 0], np.int32), np.array([5, 5, 5, 1], np.int32)


def _expected():
    ends, outside = np.zeros((2, 2, 3, 3, 2), np.int64), np.zeros((2, 2, 3), np.int64)
    CAP, TMO = 0, 1
    ends[0, CAP, 0, 0, 0] = 1       # slot 0 row 0: (10, 10)
    ends[0, CAP, 1, 1, 1] = 1       #               (40, 40)
    outside[0, CAP, 2] = 1          #               (NaN, 5)
    ends[0, CAP, 0, 2, 1] = 1       # slot 3 row 1: (64, 32)
    ends[0, CAP, 1, 0, 0] = 1       #               (0, 0)
    ends[0, CAP, 2, 0, 0] = 1       #               (31.9, 31.9)
    ends[0, TMO, 0, 2, 0] = 1       # slot 0 row 2: (70, 5)
    outside[0, TMO, 1] = 1          #               (-1, 5)
    ends[0, TMO, 2, 0, 1] = 1       #               (5, 40)
    ends[1, TMO, 0, 2, 1] = 1       # slot 1 row 1: (95, 63)
    outside[1, TMO, 1] = 1          #               (200, 10): cx = 6 >= Wc
    ends[1, TMO, 2, 1, 0] = 1       #               (33, 0)
    return ends, outside


def _ends_tracker():
    tr = PositionTracker(4, ["a0", "a1", "a2"], 2, (96, 64), 32, 2, final_positions=True)
    assert (tr.Wc, tr.Hc) == (3, 2)
    return tr


@pytest.mark.parametrize("one_by_one", [False, True], ids=["three rows at once", "row by row"])
def test_the_numpy_form_of_the_ends_update_on_hand_made_rows(one_by_one):
    from as_cops_and_thieves_amd.positions import CAPTURE, SPAWN, TIMEOUT
    assert (CAPTURE, TIMEOUT) == (0, 1)
    final, team, term, trunc, group, quota = _hand_made()
    tr = _ends_tracker()
    tr.set_groups(group)
    tr.set_quota(quota)
    f, p, t, u = (torch.from_numpy(v) for v in (final, team, term, trunc))
    if one_by_one:                                              # the quota rule holds across calls: ``done`` is carried by the tracker
        for k in range(3):
            tr.update(p[k], t[k], None, final_positions=f[k], truncated=u[k])
    else:
        tr.update(p, t, None, final_positions=f, truncated=u)
    got = tr.counts()
    ends, outside = _expected()
    assert got["ends"].dtype == np.int64 and got["ends"].shape == (2, 2, 3, 3, 2) and got["ends_outside"].shape == (2, 2, 3)
    assert np.array_equal(got["ends"], ends) and np.array_equal(got["ends_outside"], outside)
    assert got["done"].tolist() == [2, 1, 0, 1]                 # the ends update read ``done`` and left it to the positions update
    # every end counted at a valid position is a spawn of the same row, agent by agent
    assert got["counts"][:, SPAWN].sum() == 3 * 4 and ends.sum() + outside.sum() == 3 * 4
    assert got["rows"].tolist() == [3 + 2, 3]
    s = tr.summary()
    a0, a1 = s[0]["agents"]["a0"], s[0]["agents"]["a1"]
    assert (a0["captures"], a0["timeouts"], a0["top_timeout_cell"]) == (2, 1, (2, 0)) and a0["top_capture_cell"] in ((0, 0), (2, 1))
    assert (a1["captures"], a1["timeouts"], a1["top_timeout_cell"]) == (2, 0, None)
    assert s[1]["agents"]["a2"]["top_timeout_cell"] == (1, 0) and s[1]["agents"]["a2"]["top_capture_cell"] is None
    assert set(tr.tensors()) >= {"ends", "ends_outside"}
    tr.clear()
    assert all(int(v.sum()) == 0 for v in tr.counts().values())


def test_update_ends_alone_leaves_done_and_the_other_maps_alone():
    final, _, term, trunc, group, quota = _hand_made()
    tr = _ends_tracker()
    tr.set_groups(group)
    tr.set_quota(quota)
    tr.update_ends(torch.from_numpy(final), torch.from_numpy(term), torch.from_numpy(trunc).bool())
    got = tr.counts()
    ends, outside = _expected()
    assert np.array_equal(got["ends"], ends) and np.array_equal(got["ends_outside"], outside)
    assert got["done"].sum() == 0 and got["counts"].sum() == 0 and got["rows"].sum() == 0
    for bad in ((torch.zeros(4, 3, 2, dtype=torch.float16), torch.zeros(3, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8)),
                (torch.zeros(2, 4, 2, 2, dtype=torch.float16), torch.zeros(2, 4, dtype=torch.uint8), torch.zeros(2, 4, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            tr.update_ends(*bad)
    with pytest.raises(ValueError, match="go together"):
        tr.update(torch.zeros(4, 3, 2, dtype=torch.float16), torch.zeros(4, dtype=torch.uint8), final_positions=torch.zeros(4, 3, 2, dtype=torch.float16))


# ---------------------------------------------------------------------------------------------- 3. header <-> library <-> ctypes
def test_ends_header_matches_the_library_and_the_ctypes_mirror():
    from as_cops_and_thieves_amd import _learn_native as ln
    ln.build()
    L = ln.lib()
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_render.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct cat_render_positions_ends_args \{(.*?)\} cat_render_positions_ends_args;", code, re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"\b([A-Za-z_0-9]+)\s*(?=,|$)", decl.strip())]
    assert names == [f[0] for f in ln.PositionsEndsArgs._fields_], names
    assert C.sizeof(ln.PositionsEndsArgs) == 8 * 4 + 8 * 8
    assert re.search(r"\bint\s+cat_render_positions_ends_update\s*\(\s*const\s+cat_render_positions_ends_args\s*\*\s*a\s*,\s*void\s*\*\s*stream\s*\)\s*;", code)
    assert hasattr(L, "cat_render_positions_ends_update") and "cat_render_positions_ends_update" in ln.MODULES["cat_render"][1]
    assert L.cat_render_abi_version() == 1
    for name, value in (("CAPTURE", ln.POSITIONS_CAPTURE), ("TIMEOUT", ln.POSITIONS_TIMEOUT)):
        assert re.search(r"#define CAT_POSITIONS_%s %d\b" % (name, value), code), name
    # the existing struct is as it was
    assert C.sizeof(ln.PositionsArgs) == 10 * 4 + 9 * 8 and [f[0] for f in ln.PositionsArgs._fields_][-4:] == ["counts", "outside", "rows", "done"]


def test_ends_update_refuses_bad_arguments_before_touching_a_device():
    """Every call comes back with -1 and a message and never reaches a HIP call (the fake device pointers are never dereferenced)."""
    from as_cops_and_thieves_amd import _learn_native as ln
    L = ln.lib()
    fake = 0x1000

    def args(**kw):
        a = ln.PositionsEndsArgs(3, 8, 3, 8, 5, 4, 2, 0, fake, fake, fake, fake, fake, fake, fake, fake)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def rejects(a, what):
        assert L.cat_render_positions_ends_update(C.byref(a), None) == -1
        msg = L.cat_render_last_error().decode()
        assert msg.startswith("cat_render_positions_ends_update:") and what in msg, msg

    assert L.cat_render_positions_ends_update(None, None) == -1
    for kw in ({"T": 0}, {"T": 65537}, {"N": 0}, {"A": 0}, {"A": 17}):
        rejects(args(**kw), "dimensions")
    rejects(args(cell=0), "cell")
    rejects(args(Wc=0), "grid")
    rejects(args(Hc=0), "grid")
    rejects(args(G=0), "G must be")
    for name in ("final_positions", "terminated", "truncated", "ends", "ends_outside"):
        rejects(args(**{name: 0}), "NULL")
    rejects(args(final_positions=fake + 2), "aligned")


# ---------------------------------------------------------------------------------------------- 4. the heatmaps, and the old output
def _empty_map():
    return CompiledMap(name="empty", window=(96.0, 64.0), shape_bb=np.zeros((0, 4)), shape_first=np.zeros(0, np.int32), shape_count=np.zeros(0, np.int32),
                       planes=np.zeros((0, PLANE_STRIDE)), start_pos=np.zeros((3, 2)), region_off=np.zeros(4, np.int32), regions=np.zeros((0, 4)),
                       n_cops=2, n_thieves=1)


def test_write_heatmaps_writes_the_capture_and_timeout_pictures(tmp_path):
    from as_cops_and_thieves_amd.render import HEAT_PALETTE, render_heatmap, write_heatmaps
    final, team, term, trunc, group, quota = _hand_made()
    tr = _ends_tracker()
    tr.set_groups(group)
    tr.set_quota(quota)
    tr.update(*(torch.from_numpy(v) for v in (team, term)), None, final_positions=torch.from_numpy(final), truncated=torch.from_numpy(trunc))
    c = write_heatmaps(tmp_path / "hm", tr, _empty_map(), group_names=["first", "second"])
    files = sorted(p.relative_to(tmp_path / "hm").as_posix() for p in (tmp_path / "hm").rglob("*") if p.is_file())
    planes = ("occ", "seen", "hidden", "spawn", "capture", "timeout")
    assert files == sorted([f"{g}/a{i}_{p}.png" for g in ("first", "second") for i in range(3) for p in planes] + ["positions.npz"])
    z = np.load(tmp_path / "hm" / "positions.npz")
    ends, outside = _expected()
    assert np.array_equal(z["ends"], ends) and np.array_equal(z["ends_outside"], outside) and np.array_equal(c["ends"], ends)
    png = (tmp_path / "hm" / "first" / "a0_timeout.png").read_bytes()
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    img = render_heatmap(_empty_map(), ends[0, 1, 0], 32)          # the picture that file holds: cell (2, 0) at the top level, the rest empty
    assert (img[64:96, 0:32] == HEAT_PALETTE[255]).all() and (img[0:64] == HEAT_PALETTE[0]).all() and (img[64:96, 32:64] == HEAT_PALETTE[0]).all()


def test_a_tracker_without_final_positions_gives_the_old_output_key_for_key(tmp_path):
    from as_cops_and_thieves_amd.render import write_heatmaps
    _, team, term, _, group, quota = _hand_made()
    tr = PositionTracker(4, ["a0", "a1", "a2"], 2, (96, 64), 32, 2)
    tr.set_groups(group)
    tr.set_quota(quota)
    tr.update(torch.from_numpy(team), torch.from_numpy(term))
    assert list(tr.counts()) == ["counts", "outside", "rows", "done"]
    assert list(tr.tensors()) == ["counts", "outside", "rows", "done", "group", "quota"]
    assert list(tr.summary()[0]["agents"]["a0"]) == ["outside", "occupied", "seen", "spawns", "cells_visited", "seen_fraction", "top_cell", "top_hidden_cell"]
    assert tr._flat.numel() == 2 * 3 * 3 * 3 * 2 + 2 * 3 + 2 + 2            # counts, outside, rows, done: no room for anything else
    with_ends = _ends_tracker()
    with_ends.set_groups(group)
    with_ends.set_quota(quota)
    with_ends.update(torch.from_numpy(team), torch.from_numpy(term))        # built for the ends but fed none: the same counts, empty ends
    for k, v in tr.counts().items():
        assert np.array_equal(v, with_ends.counts()[k]), k
    assert with_ends.counts()["ends"].sum() == 0
    write_heatmaps(tmp_path / "hm", tr, _empty_map(), group_names=["g", None])
    files = sorted(p.relative_to(tmp_path / "hm").as_posix() for p in (tmp_path / "hm").rglob("*") if p.is_file())
    assert files == sorted([f"g/a{i}_{p}.png" for i in range(3) for p in ("occ", "seen", "hidden", "spawn")] + ["positions.npz"])
    assert sorted(np.load(tmp_path / "hm" / "positions.npz").files) == sorted(["counts", "outside", "rows", "done", "cell", "agents", "groups"])
    f = torch.zeros(4, 3, 2, dtype=torch.float16)
    with pytest.raises(ValueError, match="final_positions=True"):
        tr.update(f, torch.zeros(4, dtype=torch.uint8), None, final_positions=f, truncated=torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="final_positions=True"):
        tr.update_ends(f, torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8))


def test_the_env_option_is_checked_and_documented_without_a_device():
    import inspect
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    p = inspect.signature(VecCopsEnv.__init__).parameters["final_positions"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert "0x7E00" in VecCopsEnv.__doc__ and "NOT WRITTEN" in VecCopsEnv.__doc__
