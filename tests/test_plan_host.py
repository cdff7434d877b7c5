"""cat_create's plan without a device (cat_plan_describe_host): for every case of tests/plan_cases.py the text -- every decision (form of the ray fan,
workgroup size, LDS carve, ring, chunks per unit, kernels) and an FNV-1a 64 hash of every table that would be uploaded -- equals the text recorded from
the library as it was before plan and upload were separated (tests/golden/plan/<case>.txt, recorded on an MI355X from cat_create's own locals).  And the
refusals that need no device, each with its code and message."""
import ctypes as C
import json
import math
import re
import struct

import numpy as np
import pytest

from as_cops_and_thieves_amd import _native
from as_cops_and_thieves_amd.config import SimConfig
from as_cops_and_thieves_amd.maps import Map, load_preset
from tests import plan_cases as pc

BAD_CONFIG, BAD_MAP, BAD_SLOT_MAP = -1, -2, -3
INVALID = "map blob 0 invalid, roster mismatch or more than 256 shapes"


@pytest.mark.parametrize("name", list(pc.CASES))
def test_plan_is_the_recorded_one(name):
    want = (pc.GOLDEN / f"{name}.txt").read_text()
    got = pc.describe_case(pc.CASES[name])
    if got != want:
        a, b = want.splitlines(), got.splitlines()
        diff = [f"{x!r} -> {y!r}" for x, y in zip(a, b) if x != y]
        pytest.fail(f"{name}: {len(a)} -> {len(b)} lines; differing: {diff[:12]}")


def test_the_text_names_every_decision_and_table():
    text = pc.describe_case(pc.CASES["labyrinth_n64_pool1"])
    keys = [ln.split("=", 1)[0] for ln in text.splitlines()]
    assert len(keys) == len(set(keys)) and all("=" in ln for ln in text.splitlines())
    for k in "N A n_cops R gate NP rec_bytes hot_bytes ang_ok ang0 inv_step".split():
        assert f"sim.{k}" in keys
    for k in ("fan map_ids n_envs n_blocks wpb lds_bytes lds_map lds_env lds_union lds_racc lds_pool_off maxc maxE grp_rays item_cap pool_mask pool_magic "
              "pool_shift pool_step row_words row_id_bits row_cnt_mul csr kernel_variant one_tick_kernel rollout_kernel uniform").split():
        assert f"part0.{k}" in keys
    for k in "nx ny inv_cell span span_tick max_row".split():
        assert f"part0.map0.{k}" in keys
    for k in "geo_f64 geo_i32 maps state tree_bb tree_link tree_root".split():
        assert f"sim.hash.{k}" in keys
    for k in "grids grid_rows grid_off grid_ent cgrid_off cgrid_ent cgrid_rows work_env block_map block_desc".split():
        assert f"part0.hash.{k}" in keys
    # a short buffer gets the head of the text, the return value still is the whole length
    args = pc.CreateArgs(pc.sim_config(pc.CASES["labyrinth_n64_pool1"]), [load_preset("labyrinth").compile().to_blob()])
    buf = C.create_string_buffer(32)
    with pc.knobs({"CAT_POOL": "1"}):
        rc = _native.lib().cat_plan_describe_host(C.byref(args.cfg), C.byref(args.tab), args.arr, args.sizes, 1, None, buf, len(buf))
    assert rc == len(text) and buf.value.decode() == text[:31]


# ------------------------------------------------------------------------------------------ refusals
def _refused(cfg, blobs, slot_map_ids=None, env=None):
    with pc.knobs(env or {}):
        return pc.CreateArgs(cfg, blobs, slot_map_ids).describe()


def _json_map(tmp_path, name, rings):
    blocks = [{"type": "poly", "vs": [{"x": x, "y": y} for x, y in ring]} for ring in rings]
    agents = [{"type": "cop", "x": 20, "y": 20}, {"type": "cop", "x": 45, "y": 20}, {"type": "thief", "x": 20, "y": 45}]
    f = tmp_path / f"{name}.json"
    f.write_text(json.dumps({"window": {"w_px": 640, "h_px": 640}, "canvas": {"w": 640, "h": 640}, "objects": {"blocks": blocks}, "agents": agents}))
    return Map(f).compile()


def _ngon(cx, cy, r, n):
    return [(cx + r * math.cos(2 * math.pi * q / n), cy + r * math.sin(2 * math.pi * q / n)) for q in range(n)]


@pytest.fixture(scope="module")
def squarinth_blob():
    return load_preset("squarinth").compile().to_blob()


CFG = SimConfig(n_envs=2, n_rays=8)


def test_a_truncated_blob_and_a_wrong_magic_are_refused(squarinth_blob):
    assert _refused(CFG, [squarinth_blob[:40]]) == (BAD_MAP, "map blob 0 too small")
    assert _refused(CFG, [squarinth_blob[:-4]]) == (BAD_MAP, INVALID)
    assert _refused(CFG, [b"XXXX" + squarinth_blob[4:]]) == (BAD_MAP, INVALID)
    assert _refused(CFG, [squarinth_blob + b"\0\0\0\0"]) == (BAD_MAP, INVALID)
    # ... and the host-only entries read blobs with the same reader
    L = _native.lib()
    for blob in (squarinth_blob[:-4], b"XXXX" + squarinth_blob[4:]):
        assert L.cat_map_wall_bb_depth_host(blob, len(blob), 5.0) == BAD_MAP
        assert L.cat_bbtree_host(blob, len(blob), None, None, 0, None, None) == BAD_MAP
    assert L.cat_map_wall_bb_depth_host(squarinth_blob, len(squarinth_blob), 5.0) == 2


def test_a_roster_mismatch_is_refused(squarinth_blob):
    assert _refused(SimConfig(n_envs=2, n_rays=8, n_cops=1, n_thieves=1), [squarinth_blob]) == (BAD_MAP, INVALID)
    assert _refused(SimConfig(n_envs=2, n_rays=8, n_cops=1, n_thieves=2), [squarinth_blob]) == (BAD_MAP, INVALID)   # three agents, other teams


def test_a_wall_with_too_many_hull_edges_is_refused(squarinth_blob):
    hdr = struct.unpack("<16i", squarinth_blob[:64])
    S, P, A, Rg = hdr[2], hdr[3], hdr[4], hdr[7]
    count1 = 64 + (2 + 4 * S + 8 * P + 2 * A + 4 * Rg) * 8 + (S + 1) * 4   # plane count of wall 1
    blob = squarinth_blob[:count1] + struct.pack("<i", 32) + squarinth_blob[count1 + 4:]
    assert _refused(CFG, [blob]) == (BAD_MAP, "map blob 0: wall 1 has 32 hull edges (1..31 supported)")


def test_slot_map_ids_out_of_range_are_refused(squarinth_blob):
    assert _refused(CFG, [squarinth_blob], np.array([0, 1], np.int32)) == (BAD_SLOT_MAP, "slot_map_ids[1]=1 out of range")
    assert _refused(CFG, [squarinth_blob], np.array([-1, 0], np.int32)) == (BAD_SLOT_MAP, "slot_map_ids[0]=-1 out of range")


def test_a_deep_wall_overlap_is_refused_unless_allowed(tmp_path):
    """Nine thin walls meeting at one point: an agent's bb can overlap nine wall bbs at once, one more than the record caches."""
    hub, rings = (300.0, 300.0), []
    for q in range(9):
        dx, dy = math.cos(2 * math.pi * q / 9), math.sin(2 * math.pi * q / 9)
        p0, p1 = (hub[0] + 3 * dx, hub[1] + 3 * dy), (hub[0] + 120 * dx, hub[1] + 120 * dy)
        rings.append([(p0[0] - dy, p0[1] + dx), (p1[0] - dy, p1[1] + dx), (p1[0] + dy, p1[1] - dx), (p0[0] + dy, p0[1] - dx)])
    blob = _json_map(tmp_path, "star9", rings).to_blob()
    rc, msg = _refused(CFG, [blob])
    assert rc == BAD_MAP and msg == ("map blob 0: an agent can touch the bounding boxes of 9 walls at once; the state record caches 8 wall contacts per agent "
                                     "(CAT_WALL_CACHE); CAT_ALLOW_DEEP_WALL_OVERLAP=1 accepts the map")
    rc, text = _refused(CFG, [blob], env={"CAT_ALLOW_DEEP_WALL_OVERLAP": "1"})
    assert rc == len(text) and "part0.wall_bb_depth=9\n" in text and "part0.maxc=27\n" in text   # 3 agents x min(9, 8) walls + 3 pairs


def test_a_single_env_slot_beyond_the_lds_is_refused(tmp_path):
    """80 walls of 24 edges: bbs, plane records and edge pairs of the map alone are (6 + 8 * 24 + 10 * 12) * 8 * 80 = 203 520 bytes of the 163 840 a workgroup has."""
    rings = [_ngon(100.0 + 60.0 * (q % 10), 100.0 + 60.0 * (q // 10), 12.0, 24) for q in range(80)]
    rc, msg = _refused(CFG, [_json_map(tmp_path, "many_planes", rings).to_blob()])
    assert rc == BAD_CONFIG and re.fullmatch(r"LDS budget exceeded: (\d+) bytes for one env slot", msg), msg
    assert int(re.search(r"\d+", msg).group()) > 160 * 1024


def test_a_bad_config_is_refused_before_anything_about_the_maps():
    rc, msg = _refused(SimConfig(n_envs=2, n_rays=8, bbtree_gate=3), [b"not a map"])
    assert (rc, msg) == (BAD_CONFIG, "bad config: agents=3 rays=8 envs=2 bbtree_gate=3")
