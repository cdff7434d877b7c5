"""The batched GPU frame renderer (include/cat_render.h) against its NumPy contract (render.render_frame_reference /
render.render_rgb_array), byte for byte: VecCopsEnv.render over a mixed batch of all five maps, explicit edge positions, many frames
into a guarded buffer, the renderer's read-only promise, and the headless watch command."""
import json
import struct
import zlib

import numpy as np
import pytest
import torch

from as_cops_and_thieves_amd.environments import VecCopsEnv
from as_cops_and_thieves_amd.maps import load_preset
from as_cops_and_thieves_amd.render import render_frame_reference, render_rgb_array

pytestmark = pytest.mark.gpu

PRESETS = ("squarinth", "labyrinth", "lbirinth", "grandbyrinth", "agh-map")


def _check_frame(got: np.ndarray, want: np.ndarray, ctx: str) -> None:
    """``got`` [W_frame, H_frame, 3] must hold ``want`` [W, H, 3] in its corner and 255 everywhere else."""
    W, H = want.shape[:2]
    inside = got[:W, :H]
    if not np.array_equal(inside, want):
        diff = np.argwhere((inside != want).any(axis=2))
        x, y = diff[0]
        raise AssertionError(f"{ctx}: {len(diff)} pixels differ, first at ({x}, {y}): got {inside[x, y]}, want {want[x, y]}")
    assert (got[W:] == 255).all() and (got[:, H:] == 255).all(), f"{ctx}: pixels beyond the map window are not white"


def _env_frames_match(env, cmaps, ids, rays, ctx):
    frames = env.render(ids, rays=rays).cpu().numpy()
    pos = env.get_env_state()["pos"].cpu().numpy()
    out = env.raw_outputs()
    dist, typ = out["obs_distance"].cpu().numpy(), out["obs_type"].cpu().numpy()
    scene = env._render_scene
    n_cops = len(env.cops)
    for j, k in enumerate(ids):
        cm = cmaps[env.slot_map_ids[k]]
        if rays:
            want = render_frame_reference(cm, pos[k], n_cops, env._cfg.agent_radius, rays=scene.rays_of(dist[k], typ[k]))
        else:
            want = render_rgb_array(cm, pos[k], n_cops, env._cfg.agent_radius)
        _check_frame(frames[j], want, f"{ctx} slot {k} ({cm.name}, rays={rays})")


def test_vec_env_render_matches_numpy_on_all_five_maps():
    maps = [load_preset(n, 2, 1) for n in PRESETS]
    N = 10
    ids = [k % len(PRESETS) for k in range(N)]
    env = VecCopsEnv(maps, N, slot_map_ids=ids, num_rays=64, max_step_count=40, seed=11)
    cmaps = env._compiled
    env.reset()
    frames = env.render()
    assert frames.shape == (1, 1280, 800, 3) and frames.dtype == torch.uint8 and frames.device.type == "cuda"
    every = list(range(N))
    _env_frames_match(env, cmaps, every, False, "reset")
    _env_frames_match(env, cmaps, every, True, "reset")
    for t in range(50):                        # episodes of 40 ticks at most: some slots auto-reset on the way
        env.step(env.random_actions(t))
    env.check_errors()
    assert int(env.get_env_state()["reset_count"].max()) > 0
    _env_frames_match(env, cmaps, every, False, "tick 50")
    _env_frames_match(env, cmaps, every, True, "tick 50")
    _env_frames_match(env, cmaps, [7, 2, 2], True, "tick 50, picked slots")
    with pytest.raises(IndexError):
        env.render([N])
    env.close()


@pytest.mark.parametrize("name,roster", [("agh-map", (2, 1)), ("labyrinth", (2, 1)), ("labyrinth", (3, 2))])
def test_explicit_edge_positions(name, roster):
    from as_cops_and_thieves_amd.constants import DEFAULT_SENSOR
    from as_cops_and_thieves_amd.render_gpu import RenderScene
    cm = load_preset(name, *roster).compile()
    scene = RenderScene([cm], "cuda", sensor=DEFAULT_SENSOR)           # 90 rays: the A x R segments take two culling chunks
    A, R = cm.n_agents, scene.n_rays
    W, H = int(cm.window[0]), int(cm.window[1])
    rng = np.random.default_rng(7)
    cases = [
        [(-3.2, -4.7), (0.4, 0.6), (-0.5, 700.3)][:A] + [(5.0, 5.0)] * (A - 3),       # negative coordinates, the corner walls
        [(W + 2.5, 10.0), (W - 0.5, H - 0.5), (640.0, H + 7.25)][:A] + [(W + 50.0, H + 50.0)] * (A - 3),   # at and beyond the window
        [(300.25, 300.75)] * A,                                                        # every agent on one spot
        [(300.25 + 3 * i, 300.75 - 2 * i) for i in range(A)],                          # overlapping discs
        [(1e6, -1e6), (float(W), float(H)), (0.0, 0.0)][:A] + [(1.5, 1.5)] * (A - 3),
    ]
    pos = np.array(cases, dtype=np.float64)
    F = len(cases)
    dist = (rng.random((F, A, R)) * 400.0).astype(np.float16)
    dist[:, :, ::7] = 0.0                                                               # zero-length rays
    dist[:, :, 3::11] = 400.0
    typ = rng.integers(0, 5, size=(F, A, R)).astype(np.uint8)
    typ[0, 0, :5] = 9                                                                    # beyond the palette: drawn as EMPTY
    frames = scene.frames([0] * F, torch.from_numpy(pos), rays=(torch.from_numpy(dist).cuda(), torch.from_numpy(typ).cuda()))
    plain = scene.frames([0] * F, torch.from_numpy(pos))
    frames, plain = frames.cpu().numpy(), plain.cpu().numpy()
    for f in range(F):
        want = render_frame_reference(cm, pos[f], cm.n_cops, scene.agent_radius, rays=scene.rays_of(dist[f], typ[f]))
        _check_frame(frames[f], want, f"{name} {roster} case {f} with rays")
        _check_frame(plain[f], render_rgb_array(cm, pos[f], cm.n_cops, scene.agent_radius), f"{name} {roster} case {f}")
    if roster == (3, 2):                     # the colour split at n_cops = 3: agent 2 (the last disc over pixel 303, 299) blue, agent 3 red
        assert tuple(plain[3, 303, 299]) == (0, 0, 255) and tuple(plain[3, 307, 296]) == (255, 0, 0)


def test_many_frames_into_a_guarded_unaligned_slice():
    from as_cops_and_thieves_amd.render_gpu import RenderScene
    cms = [load_preset("squarinth", 2, 1).compile(), load_preset("agh-map", 2, 1).compile()]
    scene = RenderScene(cms, "cuda")
    F, W, H, A, R = 256, scene.width, scene.height, 3, scene.n_rays
    n = F * W * H * 3
    guard = 4099
    buf = torch.full((n + 2 * guard + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[guard + 1:guard + 1 + n].view(F, W, H, 3)                 # odd start: the kernel's byte-store path
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 2, size=F).astype(np.int32)
    pos = np.stack([rng.uniform(-20, 1300, size=(F, A)), rng.uniform(-20, 820, size=(F, A))], axis=-1)
    dist = (rng.random((F, A, R)) * 400.0).astype(np.float16)
    typ = rng.integers(0, 5, size=(F, A, R)).astype(np.uint8)
    got = scene.frames(ids, torch.from_numpy(pos), rays=(torch.from_numpy(dist).cuda(), torch.from_numpy(typ).cuda()), out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    g = buf.cpu().numpy()
    assert (g[:guard + 1] == 0xA5).all() and (g[guard + 1 + n:] == 0xA5).all(), "a guard byte was written"
    host = g[guard + 1:guard + 1 + n].reshape(F, W, H, 3)
    for f in (0, 1, 77, 128, 200, 255):
        cm = cms[ids[f]]
        want = render_frame_reference(cm, pos[f], cm.n_cops, scene.agent_radius, rays=scene.rays_of(dist[f], typ[f]))
        _check_frame(host[f], want, f"frame {f} ({cm.name})")
    aligned = scene.frames(ids, torch.from_numpy(pos), rays=(torch.from_numpy(dist).cuda(), torch.from_numpy(typ).cuda()))
    assert torch.equal(aligned, out)                                    # the dword-store path writes the same bytes


def test_rendering_is_read_only():
    maps = [load_preset("agh-map", 2, 1), load_preset("labyrinth", 2, 1)]
    envs = [VecCopsEnv(maps, 6, slot_map_ids=[0, 1, 0, 1, 0, 1], num_rays=64, max_step_count=60, seed=5) for _ in range(2)]
    for e in envs:
        e.reset()
    for t in range(100):
        outs = []
        for j, e in enumerate(envs):
            out = e.step_raw(e.random_actions(t))
            if j == 1:
                e.render(range(6), rays=True)
            outs.append({k: v.clone() for k, v in out.items()})
        for k in outs[0]:
            assert torch.equal(outs[0][k], outs[1][k]), (t, k)
    s0, s1 = envs[0].get_env_state(), envs[1].get_env_state()
    for k in s0:
        assert torch.equal(s0[k].view(torch.uint8) if s0[k].dtype == torch.float64 else s0[k],
                           s1[k].view(torch.uint8) if s1[k].dtype == torch.float64 else s1[k]), k
    for e in envs:
        e.check_errors()
        e.close()


def _read_png(path) -> np.ndarray:
    data = open(path, "rb").read()
    pos, idat, ihdr = 8, b"", None
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            ihdr = struct.unpack(">II", body[:8])
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h = ihdr
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    return raw[:, 1:].reshape(h, w, 3).transpose(1, 0, 2)


def test_watch_writes_frames_and_episodes(tmp_path):
    from as_cops_and_thieves_amd.selfplay import watch
    res = watch.watch("squarinth", 2, tmp_path, ticks=30, rays=True, seed=4, log=lambda *a: None)
    meta = json.loads((tmp_path / "episode.json").read_text())
    assert meta["envs"] == 2 and len(meta["slots"]) == 2 and meta == json.loads(json.dumps(res))
    for s in meta["slots"]:
        k = s["env"]
        frames = sorted((tmp_path / f"env_{k}").glob("frame_*.png"))
        assert len(frames) == s["frames"] and frames[0].name == "frame_00000.png"
        assert 1 <= s["length"] <= 30 and (s["winner"] in ("cop", "thief", None))
    # frame 0 is the seeded reset state: the same env, reset as often as watch resets it (the trainer once, watch once)
    env = watch.make_env("squarinth", 2, seed=4)
    env.reset()
    env.reset()
    pos = env.get_env_state()["pos"].cpu().numpy()
    out = env.raw_outputs()
    dist, typ = out["obs_distance"].cpu().numpy(), out["obs_type"].cpu().numpy()
    env.render()                                                   # builds the scene (for its ray table)
    cm = env._compiled[0]
    for k in range(2):
        want = render_frame_reference(cm, pos[k], cm.n_cops, env._cfg.agent_radius, rays=env._render_scene.rays_of(dist[k], typ[k]))
        assert np.array_equal(_read_png(tmp_path / f"env_{k}" / "frame_00000.png"), want), k
    env.close()
