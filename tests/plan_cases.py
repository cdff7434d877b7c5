"""The sims whose plan (every decision cat_create takes and a hash of every table it uploads) is pinned by tests/golden/plan/<case>.txt, and
the ctypes plumbing to ask the library for that text without a device (cat_plan_describe_host).  Shared by tests/test_plan_host.py (CPU, against the
goldens) and tests/test_gpu_plan.py (GPU: what cat_create prints under CAT_VERBOSE=1 is the same text)."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np

from as_cops_and_thieves_amd import _native, tables
from as_cops_and_thieves_amd.config import C_FIELDS_F64, C_FIELDS_I32, SimConfig
from as_cops_and_thieves_amd.maps import load_preset

GOLDEN = Path(__file__).resolve().parent / "golden" / "plan"
FIVE = ("labyrinth", "squarinth", "grandbyrinth", "lbirinth", "agh-map")


@dataclass(frozen=True)
class PlanCase:
    maps: Tuple[str, ...]
    n_cops: int
    n_thieves: int
    n_rays: int
    n_envs: int
    gate: int = 1
    slots: Optional[str] = None          # None: every slot on map 0; "interleave": slot e on map e % n_maps; "thirds": map 0 for every third slot, else map 1
    env: Dict[str, str] = field(default_factory=dict)

    def slot_map_ids(self):
        e = np.arange(self.n_envs)
        if self.slots == "interleave":
            return (e % len(self.maps)).astype(np.int32)
        if self.slots == "thirds":
            return np.where(e % 3 == 0, 0, 1).astype(np.int32)
        return None


_LAB64 = dict(maps=("labyrinth",), n_cops=2, n_thieves=1, n_rays=64, n_envs=64)
_AGH64 = dict(maps=("agh-map",), n_cops=2, n_thieves=1, n_rays=64, n_envs=64)
CASES: Dict[str, PlanCase] = {
    "squarinth_1v1_r90_n64": PlanCase(("squarinth",), 1, 1, 90, 64),
    "labyrinth_2v1_r64_n4096": PlanCase(("labyrinth",), 2, 1, 64, 4096),
    "labyrinth_2v1_r90_n4096": PlanCase(("labyrinth",), 2, 1, 90, 4096),
    "agh_2v1_r64_n4096": PlanCase(("agh-map",), 2, 1, 64, 4096),
    "grandbyrinth_3v2_r64_n8192": PlanCase(("grandbyrinth",), 3, 2, 64, 8192),
    "five_2v1_r64_n16384": PlanCase(FIVE, 2, 1, 64, 16384, slots="interleave"),
    "five_2v1_r64_n16384_split": PlanCase(FIVE, 2, 1, 64, 16384, slots="interleave", env={"CAT_SPLIT": "1"}),
    "agh_tree_n64": PlanCase(("agh-map",), 2, 1, 64, 64, gate=2),
    "squarinth_lbirinth_2v2_r32_n100": PlanCase(("squarinth", "lbirinth"), 2, 2, 32, 100, slots="thirds"),
    "labyrinth_n64_pool0": PlanCase(**_LAB64, env={"CAT_POOL": "0"}),
    "labyrinth_n64_pool1": PlanCase(**_LAB64, env={"CAT_POOL": "1"}),
    "labyrinth_n64_fan_chunks": PlanCase(**_LAB64, env={"CAT_FAN": "chunks"}),
    "labyrinth_n64_generic": PlanCase(**_LAB64, env={"CAT_GENERIC_KERNEL": "1"}),
    "labyrinth_n64_wpb3": PlanCase(**_LAB64, env={"CAT_WAVES_PER_BLOCK": "3"}),
    "agh_n64_item_cap16_chunks3": PlanCase(**_AGH64, env={"CAT_ITEM_CAP": "16", "CAT_SLOT_CHUNKS": "3"}),
    "agh_n64_grid_fields0": PlanCase(**_AGH64, env={"CAT_GRID_FIELDS": "0"}),
}


@contextlib.contextmanager
def knobs(env: Dict[str, str]):
    """The process environment with exactly these CAT_* planning knobs set (the library reads them when a plan is made)."""
    keep = ("CAT_SIM_LIB",)
    saved = {k: v for k, v in os.environ.items() if k.startswith("CAT_") and k not in keep}
    for k in saved:
        del os.environ[k]
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def compiled_maps(case: PlanCase):
    return [load_preset(m, case.n_cops, case.n_thieves).compile() for m in case.maps]


def sim_config(case: PlanCase) -> SimConfig:
    return SimConfig(n_envs=case.n_envs, n_cops=case.n_cops, n_thieves=case.n_thieves, n_rays=case.n_rays, bbtree_gate=case.gate)


class CreateArgs:
    """cat_create's / cat_plan_describe_host's arguments for (cfg, blobs, slot ids); keeps the buffers alive."""

    def __init__(self, cfg: SimConfig, blobs, slot_map_ids=None):
        self.cfg = _native.CatConfig()
        for n in C_FIELDS_I32 + C_FIELDS_F64:
            setattr(self.cfg, n, getattr(cfg, n))
        self.cfg.env_id_offset, self.cfg.seed = cfg.env_id_offset, cfg.seed
        dx, dy = tables.ray_table(cfg.sensor)
        self._host = [dx, dy, tables.cop_reward_lut(), tables.thief_reward_lut()]
        self.tab = _native.CatTables(*[a.ctypes.data_as(C.c_void_p) for a in self._host])
        self.blobs = list(blobs)
        self.arr = (C.c_char_p * len(self.blobs))(*self.blobs)
        self.sizes = (C.c_size_t * len(self.blobs))(*[len(b) for b in self.blobs])
        self.ids = None if slot_map_ids is None else np.ascontiguousarray(slot_map_ids, np.int32)

    def describe(self):
        """(return code, text): cat_plan_describe_host with a buffer that is large enough."""
        L = _native.lib()
        ids = None if self.ids is None else self.ids.ctypes.data_as(C.c_void_p)
        buf = C.create_string_buffer(1 << 16)
        rc = L.cat_plan_describe_host(C.byref(self.cfg), C.byref(self.tab), self.arr, self.sizes, len(self.blobs), ids, buf, len(buf))
        return rc, (buf.value.decode() if rc >= 0 else L.cat_last_error(None).decode())


def describe_case(case: PlanCase) -> str:
    args = CreateArgs(sim_config(case), [m.to_blob() for m in compiled_maps(case)], case.slot_map_ids())
    with knobs(case.env):
        rc, text = args.describe()
    assert rc == len(text) > 0, (rc, text)
    return text
