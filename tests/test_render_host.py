"""The batched frame renderer without a GPU: include/cat_render.h <-> libcat_learn.so <-> the ctypes mirror, the argument checks of
cat_render_frames (which come before any device call), the NumPy pixel contract (render.render_frame_reference) on hand-built
scenes, and the standard-library PNG writer."""
import ctypes as C
import re
import struct
import zlib
from pathlib import Path

import numpy as np
import pytest

from as_cops_and_thieves_amd.maps import PLANE_STRIDE, CompiledMap, load_preset
from as_cops_and_thieves_amd.render import RAY_COLOURS, render_frame_reference, render_rgb_array, write_png

ROOT = Path(__file__).resolve().parents[1]
PRESETS = ("squarinth", "labyrinth", "lbirinth", "grandbyrinth", "agh-map")
WHITE, BLUE, RED = (255, 255, 255), (0, 0, 255), (255, 0, 0)


def _empty_map(W=40, H=30, n_cops=1, n_thieves=1) -> CompiledMap:
    A = n_cops + n_thieves
    return CompiledMap(name="empty", window=(float(W), float(H)), shape_bb=np.zeros((0, 4)), shape_first=np.zeros(0, np.int32),
                       shape_count=np.zeros(0, np.int32), planes=np.zeros((0, PLANE_STRIDE)), start_pos=np.zeros((A, 2)),
                       region_off=np.zeros(A + 1, np.int32), regions=np.zeros((0, 4)), n_cops=n_cops, n_thieves=n_thieves)


def _rays(dx, dy, length, dist, types):
    return (np.asarray(dx, np.float64), np.asarray(dy, np.float64), float(length),
            np.asarray(dist, np.float16), np.asarray(types, np.uint8))


def _lit(img, colour):
    return set(zip(*np.nonzero((img == np.array(colour, np.uint8)).all(axis=2))))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_render_header_library_and_ctypes_mirror_agree():
    from as_cops_and_thieves_amd import _learn_native as ln
    ln.build()
    L = ln.lib()
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cat_render.h").read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cat_render_[a-z_0-9]+)\s*\(", code)))
    assert set(declared) == set(ln.RENDER_SYMBOLS) and all(hasattr(L, s) for s in declared)
    for struct_name, cls in (("cat_render_scene", ln.RenderSceneDesc), ("cat_render_args", ln.RenderArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), code, re.S).group(1)
        body = re.sub(r"\[[^\]]*\]", "", body)
        names = [n for decl in body.split(";") for n in re.findall(r"\b([A-Za-z_0-9]+)\s*(?=,|$)", decl.strip())]
        assert names == [f[0] for f in cls._fields_], (struct_name, names)
    assert C.sizeof(ln.RenderArgs) == 8 * 4 + 2 * 8 + 6 * 8
    assert L.cat_render_abi_version() == 1
    assert "#define CAT_RENDER_RAYS %d" % ln.RENDER_RAYS in code
    pal = re.search(r"CAT_RENDER_RAY_COLOURS \{(.*)\}", code).group(1)
    assert [tuple(map(int, t)) for t in re.findall(r"\{(\d+), (\d+), (\d+)\}", pal)] == [tuple(c) for c in RAY_COLOURS.tolist()]
    for f in ("render.py", "render_gpu.py"):       # the learner library's sources and headers include the renderer
        assert (ROOT / "as_cops_and_thieves_amd" / f).exists()
    assert ROOT / "as_cops_and_thieves_amd" / "csrc" / "cat_render.hip" in ln.SOURCES
    assert ROOT / "include" / "cat_render.h" in ln.HEADERS


def test_render_frames_rejects_bad_arguments_before_touching_a_device():
    """Host-pointer-only arguments: every call below must come back with -1 and a message and never reach a HIP call (there is no
    device here; the fake device pointers are never dereferenced)."""
    from as_cops_and_thieves_amd import _learn_native as ln
    L = ln.lib()
    fake = 0x1000                                          # a non-NULL stand-in for a device buffer
    win = np.array([[40, 30], [64, 20]], np.int32)
    off = np.array([0, 0, 0], np.int32)
    scene = ln.RenderSceneDesc(2, 8, fake, win.ctypes.data, fake, off.ctypes.data, fake, fake, fake, fake, fake, fake)
    ids = np.array([0, 1], np.int32)

    def args(**kw):
        a = ln.RenderArgs(2, 64, 30, 0, 1, 2, 8, 0, 5.0, 400.0, ids.ctypes.data, fake, fake, 0, 0, fake)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def rejects(a, what, sc=scene):
        assert L.cat_render_frames(C.byref(sc), C.byref(a), None) == -1
        msg = L.cat_render_last_error().decode()
        assert msg.startswith("cat_render_frames:") and what in msg, msg

    assert L.cat_render_frames(None, C.byref(args()), None) == -1
    rejects(args(F=0), "dimensions")
    rejects(args(width=0), "dimensions")
    rejects(args(A=0), "dimensions")
    rejects(args(A=17), "dimensions")
    rejects(args(n_cops=3), "dimensions")
    rejects(args(agent_radius=float("nan")), "agent_radius")
    rejects(args(flags=2), "flags")
    rejects(args(flags=1), "obs_distance")                 # rays without the observation buffers
    rejects(args(flags=1, R=7, obs_distance=fake, obs_type=fake), "ray table")
    rejects(args(flags=1, ray_length=0.0, obs_distance=fake, obs_type=fake), "ray_length")
    rejects(args(positions=0), "NULL")
    rejects(args(map_ids_dev=0), "NULL")
    rejects(args(frames=0), "NULL")
    bad = np.array([0, 2], np.int32)
    rejects(args(map_ids=bad.ctypes.data), "map_ids[1] = 2")
    neg = np.array([-1, 0], np.int32)
    rejects(args(map_ids=neg.ctypes.data), "map_ids[0] = -1")
    rejects(args(width=63), "exceeds the frame size")      # map 1 is 64 wide
    rejects(args(height=29), "exceeds the frame size")     # map 0 is 30 high
    incomplete = ln.RenderSceneDesc(2, 8, fake, win.ctypes.data, fake, off.ctypes.data, 0, fake, fake, fake, fake, fake)
    rejects(args(), "incomplete scene", sc=incomplete)


# ---- the pixel contract ---------------------------------------------------------------------------------------------------------
def test_rays_none_is_render_rgb_array_on_every_preset():
    for name in PRESETS:
        cm = load_preset(name).compile()
        pos = cm.start_pos + np.array([0.37, -0.21])
        assert np.array_equal(render_frame_reference(cm, pos, cm.n_cops, 5.0), render_rgb_array(cm, pos, cm.n_cops, 5.0)), name


def test_ray_along_x_lights_exactly_the_expected_rows():
    cm = _empty_map(60, 30)
    pos = np.array([[10.5, 12.5], [55.0, 28.0]])        # agent 1 far away, with a zero-length ray
    img = render_frame_reference(cm, pos, 1, 0.0, rays=_rays([40.0], [0.0], 40.0, [[20.0], [0.0]], [[0], [4]]))
    wall = _lit(img, RAY_COLOURS[0])
    # the segment (10.5, 12.5) - (30.5, 12.5): pixel centres (x + .5, 12.5) for x = 10 .. 30, and no other row: the rows y = 12 +- 1
    # have their centres 1.0 away.  The radius-0 disc covers the one pixel whose centre is the agent's position, the ray's start.
    assert wall == {(x, 12) for x in range(11, 31)}
    assert _lit(img, BLUE) == {(10, 12)}


def test_zero_length_ray_lights_only_the_pixels_around_the_centre():
    cm = _empty_map(30, 30)
    pos = np.array([[15.0, 15.0], [3.0, 3.0]])          # on a pixel corner: the four pixels around it are 0.5 * sqrt(2) away (> 0.5)
    img = render_frame_reference(cm, pos, 1, 0.0, rays=_rays([40.0, 0.0], [0.0, 40.0], 40.0, [[0.0, 0.0], [0.0, 0.0]], [[1, 1], [2, 2]]))
    assert _lit(img, RAY_COLOURS[1]) == set() and _lit(img, RAY_COLOURS[2]) == set()
    pos = np.array([[15.5, 15.5], [3.5, 3.2]])          # on a pixel centre (covered by the radius-0 disc), 0.3 from one
    img = render_frame_reference(cm, pos, 0, 0.0, rays=_rays([40.0], [0.0], 40.0, [[0.0], [0.0]], [[1], [2]]))
    assert _lit(img, RAY_COLOURS[1]) == set() and _lit(img, RED) == {(15, 15)}
    assert _lit(img, RAY_COLOURS[2]) == {(3, 3)}        # the neighbours' centres are 0.7 and more away


def test_a_later_agents_ray_overwrites_an_earlier_ones():
    cm = _empty_map(60, 30)
    pos = np.array([[5.5, 10.5], [30.5, 10.5]])         # agent 0's ray runs right across agent 1's ray, which runs left
    rays = _rays([50.0], [0.0], 50.0, [[40.0], [20.0]], [[0], [3]])
    img = render_frame_reference(cm, pos, 1, 0.0, rays=rays)                # radius-0 discs: the pixels (5, 10) and (30, 10)
    assert _lit(img, RAY_COLOURS[3]) == {(x, 10) for x in range(31, 51)}
    assert _lit(img, RAY_COLOURS[0]) == {(x, 10) for x in range(6, 30)}
    rays_rev = _rays([50.0], [0.0], 50.0, [[40.0], [20.0]], [[3], [0]])      # same segments, colours exchanged: agent 1 still on top
    img2 = render_frame_reference(cm, pos, 1, 0.0, rays=rays_rev)
    assert _lit(img2, RAY_COLOURS[0]) == {(x, 10) for x in range(31, 51)}
    # within one agent, a later ray overwrites an earlier one
    pos1 = np.array([[10.5, 10.5], [50.0, 25.0]])
    img3 = render_frame_reference(cm, pos1, 1, 0.0, rays=_rays([32.0, 32.0], [0.0, 0.0], 32.0, [[32.0, 8.0], [0.0, 0.0]],
                                                                [[0, 2], [4, 4]]))
    assert _lit(img3, RAY_COLOURS[2]) == {(x, 10) for x in range(11, 19)}
    assert _lit(img3, RAY_COLOURS[0]) == {(x, 10) for x in range(19, 43)}


def test_discs_cover_ray_starts_and_walls_lie_under_rays():
    cm = load_preset("squarinth").compile()
    pos = cm.start_pos.copy()
    A = pos.shape[0]
    R = 16
    ang = np.linspace(0, 2 * np.pi, R, endpoint=False)
    rays = _rays(400 * np.cos(ang), 400 * np.sin(ang), 400.0, np.full((A, R), 60.0), np.tile(np.arange(R) % 5, (A, 1)))
    img = render_frame_reference(cm, pos, cm.n_cops, 5.0, rays=rays)
    plain = render_rgb_array(cm, pos, cm.n_cops, 5.0)
    disc = (plain == np.array(BLUE, np.uint8)).all(axis=2) | (plain == np.array(RED, np.uint8)).all(axis=2)
    assert disc.sum() > 0 and np.array_equal(img[disc], plain[disc])           # every disc pixel is the disc's colour
    changed = (img != plain).any(axis=2)
    assert changed.sum() > 0 and not (changed & disc).any()
    palette = {tuple(c) for c in RAY_COLOURS.tolist()}
    assert all(tuple(v) in palette for v in img[changed].tolist())             # everything else that changed is a ray


def test_ray_windows_clip_at_the_frame_edges():
    cm = _empty_map(20, 20)
    pos = np.array([[-5.5, 10.5], [25.5, 3.5]])                                 # both agents outside the frame
    img = render_frame_reference(cm, pos, 1, 5.0, rays=_rays([50.0], [0.0], 50.0, [[20.0], [50.0]], [[0], [1]]))
    assert _lit(img, RAY_COLOURS[0]) == {(x, 10) for x in range(0, 15)}
    assert _lit(img, RAY_COLOURS[1]) == set()                                     # agent 1's ray points away from the frame
    assert img.shape == (20, 20, 3)


def test_write_png_round_trips(tmp_path):
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, size=(37, 23, 3), dtype=np.uint8)
    path = tmp_path / "f.png"
    write_png(path, frame)
    data = path.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.setdefault(tag, b"")
        chunks[tag] += body
        pos += 12 + n
    assert list(chunks)[-1] == b"IEND"
    w, h, depth, colour, comp, filt, inter = struct.unpack(">IIBBBBB", chunks[b"IHDR"])
    assert (w, h, depth, colour, comp, filt, inter) == (37, 23, 8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    assert np.array_equal(raw[:, 1:].reshape(h, w, 3).transpose(1, 0, 2), frame)
    with pytest.raises(ValueError):
        write_png(path, frame.astype(np.float32))
