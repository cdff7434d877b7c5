"""ctypes binding of libcat_learn.so, one module per header under include/: the learner's LSTM recurrence (cat_lstm.h), convolutional trunk
(cat_trunk.h), PPO loss / optimiser step / GAE scan (cat_ppo.h) and dense layers (cat_dense.h), the rollout tick's glue (cat_rollout.h), the
batched frame renderer (cat_render.h), on-device episode accounting (cat_episodes.h) and the fused act tick (cat_act.h).  ``MODULES`` is the
one table of their entries.  No CPU fallback inside: callers on a CUDA/HIP device in bf16 get these kernels or an exception."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
LIB_PATH = PKG / "libcat_learn.so"
if os.environ.get("CAT_LEARN_LIB"):         # diagnostic builds (A/B of kernel variants): another build of the same sources
    LIB_PATH = Path(os.environ["CAT_LEARN_LIB"]).resolve()
SOURCES = tuple(PKG / "csrc" / f"cat_{n}.hip" for n in ("lstm", "trunk", "ppo", "dense", "rollout", "render", "episodes", "act"))
HEADERS = tuple(ROOT / "include" / f"cat_{n}.h" for n in ("lstm", "trunk", "ppo", "dense", "rollout", "render", "episodes", "act"))
# what the sources share, and the navigation kernels of cat_render.hip; not part of the C ABI, but inputs of the build
INTERNAL_HEADERS = (PKG / "csrc" / "cat_learn_common.h", PKG / "csrc" / "cat_render_nav.h")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-shared"]
HIDDEN = 128

_ENTRY = (C.c_int, [C.c_void_p, C.c_void_p])   # int entry(const args *, void *stream): most of the library
_QUERY = (C.c_int, [C.c_void_p])               # int query(const dims *)
# module -> (expected ABI version, {symbol: (restype, argtypes)} in the header's order); every module also has <module>_abi_version
# and <module>_last_error.  ``lib`` declares the library from this table and ``_check`` finds a symbol's error string through it.
MODULES = {
    "cat_lstm": (1, {"cat_lstm_blocks": _QUERY, "cat_lstm_saved_acts_bytes": (C.c_size_t, [C.c_void_p]),
                     "cat_lstm_saved_cell_bytes": (C.c_size_t, [C.c_void_p]), "cat_lstm_seq_forward": _ENTRY, "cat_lstm_seq_backward": _ENTRY}),
    "cat_trunk": (2, {"cat_trunk_out_positions": _QUERY, "cat_trunk_supported": _QUERY, "cat_trunk_backward_blocks": _QUERY,
                      "cat_trunk_forward": _ENTRY, "cat_trunk_backward": _ENTRY, "cat_trunk_grad_finish": _ENTRY}),
    "cat_ppo": (2, {"cat_ppo_loss_grad": _ENTRY, "cat_ppo_adam_step": _ENTRY, "cat_ppo_gae_scan": _ENTRY, "cat_ppo_gae_scan_scaled": _ENTRY,
                    "cat_ppo_moment_chunks": (C.c_int, [C.c_int32]), "cat_ppo_moments": _ENTRY,
                    "cat_ppo_loss_grad_dev": _ENTRY, "cat_ppo_adam_step_dev": _ENTRY, "cat_ppo_schedule_step": _ENTRY}),
    "cat_dense": (2, {"cat_dense_bias_act": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
                      "cat_dense_act_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
                      "cat_dense_sum_chunks": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                         C.c_int32, C.c_void_p]),
                      "cat_dense_wgrad_splits": (C.c_int, [C.c_int32] * 4), "cat_dense_wgrad": _ENTRY, "cat_dense_forward": _ENTRY,
                      "cat_dense_dgrad": _ENTRY, "cat_dense_sum_chunks2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p])}),
    "cat_rollout": (1, {"cat_rollout_pack": _ENTRY, "cat_rollout_sample": _ENTRY, "cat_rollout_post": _ENTRY, "cat_rollout_scripted": _ENTRY}),
    "cat_render": (1, {"cat_render_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]), "cat_render_positions_update": _ENTRY,
                        "cat_render_positions_ends_update": _ENTRY, "cat_render_nav_build": _ENTRY, "cat_render_nav_step": _ENTRY,
                        "cat_render_nav_shape": _ENTRY, "cat_render_nav_spawn": _ENTRY}),
    "cat_episodes": (1, {"cat_episodes_update": _ENTRY, "cat_episodes_summary": _ENTRY, "cat_episode_windows_update": _ENTRY,
                         "cat_episodes_segment_summary": _ENTRY}),
    "cat_act": (1, {"cat_act_supported": _QUERY, "cat_act_step": _ENTRY, "cat_act_collect_step": _ENTRY, "cat_act_league_step": _ENTRY}),
}
_MODULE_OF = {sym: mod for mod, (_, entries) in MODULES.items() for sym in entries}


def _symbols(module: str) -> tuple:
    return (f"{module}_abi_version", f"{module}_last_error", *MODULES[module][1])


EXPORTED_SYMBOLS = _symbols("cat_lstm")
TRUNK_SYMBOLS = _symbols("cat_trunk")


class Dims(C.Structure):
    _fields_ = [("G", C.c_int32), ("T", C.c_int32), ("B", C.c_int32), ("pad", C.c_int32)]


class FwdArgs(C.Structure):
    _fields_ = [("d", Dims), ("xproj", C.c_void_p), ("sx_g", C.c_int64), ("sx_t", C.c_int64), ("sx_b", C.c_int64),
                ("bias", C.c_void_p), ("sb_g", C.c_int64), ("bias2", C.c_void_p), ("sb2_g", C.c_int64), ("w_hh", C.c_void_p), ("sw_g", C.c_int64), ("h0", C.c_void_p), ("c0", C.c_void_p), ("keep", C.c_void_p),
                ("out", C.c_void_p), ("so_g", C.c_int64), ("so_t", C.c_int64), ("so_b", C.c_int64),
                ("h_last", C.c_void_p), ("c_last", C.c_void_p), ("h_in", C.c_void_p), ("saved_acts", C.c_void_p),
                ("saved_cell", C.c_void_p)]


class BwdArgs(C.Structure):
    _fields_ = [("d", Dims), ("d_out", C.c_void_p), ("so_g", C.c_int64), ("so_t", C.c_int64), ("so_b", C.c_int64),
                ("d_h_last", C.c_void_p), ("d_c_last", C.c_void_p), ("w_hh", C.c_void_p), ("sw_g", C.c_int64),
                ("keep", C.c_void_p), ("saved_acts", C.c_void_p), ("saved_cell", C.c_void_p),
                ("d_xproj", C.c_void_p), ("sx_g", C.c_int64), ("sx_t", C.c_int64), ("sx_b", C.c_int64),
                ("d_h0", C.c_void_p), ("d_c0", C.c_void_p), ("part_dbias", C.c_void_p)]


class TrunkDims(C.Structure):
    _fields_ = [("G", C.c_int32), ("N", C.c_int32), ("C", C.c_int32), ("R", C.c_int32)]


class TrunkParams(C.Structure):
    _fields_ = [("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("sw1_g", C.c_int64), ("sb1_g", C.c_int64), ("sw2_g", C.c_int64), ("sb2_g", C.c_int64)]


class TrunkRows(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("sel", C.c_int32), ("block", C.c_int32)]


class TrunkFwd(C.Structure):
    _fields_ = [("d", TrunkDims), ("p", TrunkParams), ("x", C.c_void_p), ("sx_g", C.c_int64), ("sx_n", C.c_int64), ("x_rows", TrunkRows),
                ("out", C.c_void_p), ("so_g", C.c_int64), ("so_n", C.c_int64)]


class TrunkBwd(C.Structure):
    _fields_ = [("d", TrunkDims), ("p", TrunkParams), ("x", C.c_void_p), ("sx_g", C.c_int64), ("sx_n", C.c_int64), ("x_rows", TrunkRows),
                ("out", C.c_void_p), ("d_out", C.c_void_p), ("so_g", C.c_int64), ("so_n", C.c_int64),
                ("part_dw1", C.c_void_p), ("part_db1", C.c_void_p), ("part_dw2", C.c_void_p), ("part_db2", C.c_void_p)]


ROLLOUT_SYMBOLS = _symbols("cat_rollout")
DENSE_SYMBOLS = _symbols("cat_dense")
PPO_SYMBOLS = _symbols("cat_ppo")
RENDER_SYMBOLS = _symbols("cat_render")
EPISODES_SYMBOLS = _symbols("cat_episodes")[:4]
EPISODE_WINDOWS_SYMBOLS = ("cat_episode_windows_update",)     # include/cat_episodes.h: the update for rows of several env ticks
EPISODE_SEGMENTS_SYMBOLS = ("cat_episodes_segment_summary",)  # include/cat_episodes.h: one summary block per contiguous segment of the slots
ACT_SYMBOLS = _symbols("cat_act")
ACT_MAX_AGENTS = 8              # CAT_ACT_MAX_AGENTS
ACT_MAX_SEGMENTS = 32           # CAT_ACT_MAX_SEGMENTS
ACT_SAMPLE, ACT_GREEDY = 0, 1   # cat_act_args.mode
EPISODES_MAX_AGENTS = 8         # CAT_ROLLOUT_MAX_AGENTS
EPISODES_HIST_BINS = 64
EPISODES_MAX_SEGMENTS = 32      # CAT_EPISODES_MAX_SEGMENTS (= ACT_MAX_SEGMENTS)
EPISODES_MAX_TICKS = 65536      # of one cat_episodes_update launch (= CAT_MAX_ROLLOUT_TICKS)
RENDER_RAYS = 1                 # cat_render_args.flags
RENDER_MAX_AGENTS = 16


class RenderSceneDesc(C.Structure):
    """include/cat_render.h cat_render_scene (device pointers except the two *_host arrays)."""
    _fields_ = [("n_maps", C.c_int32), ("n_rays", C.c_int32), ("window", C.c_void_p), ("window_host", C.c_void_p),
                ("shape_off", C.c_void_p), ("shape_off_host", C.c_void_p), ("shape_bb", C.c_void_p), ("shape_first", C.c_void_p),
                ("shape_count", C.c_void_p), ("planes", C.c_void_p), ("ray_dx", C.c_void_p), ("ray_dy", C.c_void_p)]


class RenderArgs(C.Structure):
    """include/cat_render.h cat_render_args."""
    _fields_ = [("F", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("flags", C.c_int32),
                ("n_cops", C.c_int32), ("A", C.c_int32), ("R", C.c_int32), ("pad", C.c_int32),
                ("agent_radius", C.c_double), ("ray_length", C.c_double),
                ("map_ids", C.c_void_p), ("map_ids_dev", C.c_void_p), ("positions", C.c_void_p), ("obs_distance", C.c_void_p),
                ("obs_type", C.c_void_p), ("frames", C.c_void_p)]


class PpoLoss(C.Structure):
    _fields_ = [("G", C.c_int32), ("M", C.c_int32), ("chunks", C.c_int32), ("pad", C.c_int32),
                ("logits", C.c_void_p), ("values", C.c_void_p), ("actions", C.c_void_p),
                ("old_logp", C.c_void_p), ("adv", C.c_void_p), ("ret", C.c_void_p),
                ("ratio_clip", C.c_float), ("value_scale", C.c_float), ("entropy_scale", C.c_float), ("pad2", C.c_float),
                ("d_logits", C.c_void_p), ("d_values", C.c_void_p), ("partial", C.c_void_p)]


class PpoAdam(C.Structure):
    _fields_ = [("G", C.c_int32), ("P", C.c_int32), ("chunks", C.c_int32), ("pad", C.c_int32),
                ("ar", C.c_void_p), ("col_train", C.c_void_p), ("epoch_active", C.c_void_p),
                ("m", C.c_void_p), ("v", C.c_void_p), ("steps", C.c_void_p), ("master", C.c_void_p), ("lp", C.c_void_p),
                ("kl_out", C.c_void_p), ("norm_partial", C.c_void_p),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("grad_norm_clip", C.c_float), ("kl_threshold", C.c_float)]


class PpoLossDev(C.Structure):
    _fields_ = PpoLoss._fields_ + [("hyper", C.c_void_p)]


class PpoAdamDev(C.Structure):
    _fields_ = PpoAdam._fields_ + [("hyper", C.c_void_p)]


class PpoSchedule(C.Structure):
    _fields_ = [("G", C.c_int32), ("mode", C.c_int32), ("anneal_mask", C.c_int32), ("pad", C.c_int32),
                ("hyper", C.c_void_p), ("sched_active", C.c_void_p),
                ("kl_target", C.c_float), ("kl_factor", C.c_float), ("lr_factor", C.c_float), ("lr_min", C.c_float), ("lr_max", C.c_float),
                ("progress", C.c_float),
                ("lr0", C.c_float), ("lr1", C.c_float), ("ent0", C.c_float), ("ent1", C.c_float), ("clip0", C.c_float), ("clip1", C.c_float)]


class TrunkFinish(C.Structure):
    _fields_ = [("d", TrunkDims), ("blocks", C.c_int32), ("accumulate", C.c_int32),
                ("part_dw1", C.c_void_p), ("part_db1", C.c_void_p), ("part_dw2", C.c_void_p), ("part_db2", C.c_void_p),
                ("dw1", C.c_void_p), ("db1", C.c_void_p), ("dw2", C.c_void_p), ("db2", C.c_void_p),
                ("sw1_g", C.c_int64), ("sb1_g", C.c_int64), ("sw2_g", C.c_int64), ("sb2_g", C.c_int64)]


class NativeLibraryMissing(RuntimeError):
    pass


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile the kernels in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    newest = max(f.stat().st_mtime for f in SOURCES + HEADERS + INTERNAL_HEADERS)
    stale = not LIB_PATH.exists() or LIB_PATH.stat().st_mtime < newest
    if force or stale:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc, *HIPCC_FLAGS, f"-I{ROOT / 'include'}", "-o", str(LIB_PATH), *map(str, SOURCES)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if verbose or res.returncode != 0:
            print(" ".join(cmd))
            print(res.stdout, res.stderr)
        if res.returncode != 0:
            raise RuntimeError("hipcc failed building libcat_learn.so")
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise NativeLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
                "The bf16 learner on a GPU has no other LSTM path.")
        import torch  # noqa: F401  (torch's HIP runtime first, as in _native.lib)
        L = C.CDLL(str(LIB_PATH))
        for module, (abi, entries) in MODULES.items():
            getattr(L, f"{module}_last_error").restype = C.c_char_p
            for sym, (restype, argtypes) in entries.items():
                getattr(L, sym).restype, getattr(L, sym).argtypes = restype, argtypes
            assert getattr(L, f"{module}_abi_version")() == abi, module
        _lib = L
    return _lib


def _check(rc: int, symbol: str) -> None:
    """Raise on a non-zero return of entry ``symbol`` with its module's error string."""
    if rc != 0:
        err = getattr(lib(), f"{_MODULE_OF[symbol]}_last_error")()
        raise RuntimeError(f"{symbol} failed ({rc}): {err.decode()}")


def _ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def saved_sizes(G: int, T: int, B: int):
    d = Dims(G, T, B, 0)
    return lib().cat_lstm_saved_acts_bytes(C.byref(d)), lib().cat_lstm_saved_cell_bytes(C.byref(d))


def seq_forward(xproj, w_hh, bias, h0, c0, keep, save: bool, state_out=None, bias2=None):
    """xproj bf16 [G, T, B, 4H] (any outer strides), w_hh bf16 [G, 4H, H] (rows contiguous), bias bf16 [G, 4H] or None,
    h0/c0 bf16 [G, B, H], keep fp32 [T, B] or None.  Returns out [G, T, B, H], h_T, c_T and, with ``save``, (h_in, acts, cell) for backward."""
    import torch
    G, T, B, H4 = xproj.shape
    assert H4 == 4 * HIDDEN and xproj.dtype == torch.bfloat16 and xproj.stride(3) == 1
    assert w_hh.shape == (G, H4, HIDDEN) and w_hh.dtype == torch.bfloat16 and w_hh.stride(1) == HIDDEN and w_hh.stride(2) == 1
    h0, c0 = h0.contiguous(), c0.contiguous()
    assert h0.shape == (G, B, HIDDEN) and c0.shape == h0.shape and h0.dtype == c0.dtype == torch.bfloat16
    if keep is not None:
        assert keep.shape == (T, B) and keep.dtype == torch.float32 and keep.is_contiguous()
    dev = xproj.device
    out = torch.empty(G, T, B, HIDDEN, dtype=torch.bfloat16, device=dev)
    if state_out is not None:   # written where the caller keeps the state (may be h0 / c0 themselves: a workgroup reads its
        hT, cT = state_out      # rows of the initial state before it writes the final one)
        assert hT.shape == h0.shape and cT.shape == h0.shape and hT.dtype == cT.dtype == torch.bfloat16 and hT.is_contiguous() and cT.is_contiguous()
    else:
        hT, cT = torch.empty_like(h0), torch.empty_like(c0)
    h_in = acts = cell = None
    if save:
        na, nc = saved_sizes(G, T, B)
        h_in = torch.empty(G, T, B, HIDDEN, dtype=torch.bfloat16, device=dev)
        acts = torch.empty(na, dtype=torch.uint8, device=dev)
        cell = torch.empty(nc, dtype=torch.uint8, device=dev)
    for bv in (bias, bias2):
        assert bv is None or (bv.shape == (G, H4) and bv.dtype == torch.bfloat16 and bv.stride(1) == 1)
    assert bias2 is None or bias is not None
    a = FwdArgs(Dims(G, T, B, 0), xproj.data_ptr(), xproj.stride(0), xproj.stride(1), xproj.stride(2),
                _ptr(bias), 0 if bias is None else bias.stride(0), _ptr(bias2), 0 if bias2 is None else bias2.stride(0), w_hh.data_ptr(), w_hh.stride(0), h0.data_ptr(), c0.data_ptr(), _ptr(keep),
                out.data_ptr(), out.stride(0), out.stride(1), out.stride(2), hT.data_ptr(), cT.data_ptr(),
                _ptr(h_in), _ptr(acts), _ptr(cell))
    _check(lib().cat_lstm_seq_forward(C.byref(a), _stream()), "cat_lstm_seq_forward")
    return out, hT, cT, (h_in, acts, cell)


def seq_backward(d_out, d_hT, d_cT, w_hh, keep, acts, cell, dims, want_state_grads: bool, want_bias_grad: bool = False):
    """Gradients of seq_forward: d_xproj [G, T, B, 4H], if wanted d_h0 / d_c0, and if wanted the per-workgroup partial sums
    [G, blocks, 4H] of the bias gradient."""
    import torch
    G, T, B = dims
    dev = w_hh.device
    if d_out is not None:
        assert d_out.shape == (G, T, B, HIDDEN) and d_out.dtype == torch.bfloat16
        if d_out.stride(3) != 1:
            d_out = d_out.contiguous()
    d_hT = None if d_hT is None else d_hT.contiguous()
    d_cT = None if d_cT is None else d_cT.contiguous()
    d_x = torch.empty(G, T, B, 4 * HIDDEN, dtype=torch.bfloat16, device=dev)
    d_h0 = torch.empty(G, B, HIDDEN, dtype=torch.bfloat16, device=dev) if want_state_grads else None
    d_c0 = torch.empty(G, B, HIDDEN, dtype=torch.bfloat16, device=dev) if want_state_grads else None
    part = None
    if want_bias_grad:
        dd = Dims(G, T, B, 0)
        part = torch.empty(G, lib().cat_lstm_blocks(C.byref(dd)), 4 * HIDDEN, dtype=torch.float32, device=dev)
    so = (0, 0, 0) if d_out is None else d_out.stride()[:3]
    a = BwdArgs(Dims(G, T, B, 0), _ptr(d_out), so[0], so[1], so[2], _ptr(d_hT), _ptr(d_cT), w_hh.data_ptr(), w_hh.stride(0),
                _ptr(keep), acts.data_ptr(), cell.data_ptr(), d_x.data_ptr(), d_x.stride(0), d_x.stride(1), d_x.stride(2),
                _ptr(d_h0), _ptr(d_c0), _ptr(part))
    _check(lib().cat_lstm_seq_backward(C.byref(a), _stream()), "cat_lstm_seq_backward")
    return d_x, d_h0, d_c0, part


# ---------------------------------------------------------------------------------------------- convolutional trunk
def trunk_supported(G: int, N: int, C_in: int, R: int) -> bool:
    d = TrunkDims(G, N, C_in, R)
    return bool(lib().cat_trunk_supported(C.byref(d)))


def _trunk_params(w1, b1, w2, b2, G: int, C_in: int) -> TrunkParams:
    import torch
    assert w1.shape == (G, 64, C_in, 5) and w1[0].is_contiguous() and b1.shape == (G, 64) and b1.stride(1) == 1
    assert w2.shape == (G, 32, 64, 5) and w2[0].is_contiguous() and b2.shape == (G, 32) and b2.stride(1) == 1
    assert all(t.dtype == torch.bfloat16 for t in (w1, b1, w2, b2))
    return TrunkParams(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w1.stride(0), b1.stride(0), w2.stride(0), b2.stride(0))


def _trunk_rows(x, rows, block: int):
    """(samples N, cat_trunk_rows) of an input [G, rows of x, C * R]: all of them, or -- ``rows`` int64 [sel] on the device,
    ``block`` -- the minibatch of ``sel`` sequences out of ``block`` per step, read in place (include/cat_trunk.h)."""
    import torch
    if rows is None:
        return x.shape[1], TrunkRows(None, 0, 0)
    assert rows.dtype == torch.int64 and rows.is_contiguous() and rows.device == x.device and rows.dim() == 1
    sel = rows.shape[0]
    assert 0 < sel <= block and x.shape[1] % block == 0
    return (x.shape[1] // block) * sel, TrunkRows(rows.data_ptr(), sel, block)


def trunk_forward(x, w1, b1, w2, b2, R: int, rows=None, block: int = 0):
    """x bf16 [G, N, C * R] in (channel, ray) order -> bf16 [G, N, L2 * 32] in (position, channel) order.  With ``rows``: x is
    the whole [G, steps * block, C * R] buffer and N = steps * len(rows) (``_trunk_rows``)."""
    import torch
    G, _, CR = x.shape
    C_in = CR // R
    assert x.dtype == torch.bfloat16 and x.stride(2) == 1 and C_in * R == CR
    N, xr = _trunk_rows(x, rows, block)
    d = TrunkDims(G, N, C_in, R)
    L2 = lib().cat_trunk_out_positions(C.byref(d))
    out = torch.empty(G, N, L2 * 32, dtype=torch.bfloat16, device=x.device)
    a = TrunkFwd(d, _trunk_params(w1, b1, w2, b2, G, C_in), x.data_ptr(), x.stride(0), x.stride(1), xr, out.data_ptr(), out.stride(0), out.stride(1))
    _check(lib().cat_trunk_forward(C.byref(a), _stream()), "cat_trunk_forward")
    return out


def trunk_backward(x, w1, b1, w2, b2, out, d_out, R: int, rows=None, block: int = 0):
    """fp32 per-workgroup partial sums [G, B, 64, 32], [G, B, 64], [G, B, 32, 320], [G, B, 32] of the parameter gradients
    (columns kk * C + c and kk * 64 + c_in): the caller adds the B slabs up.  ``rows``, ``block``: as in ``trunk_forward``."""
    import torch
    G, _, CR = x.shape
    C_in = CR // R
    N, xr = _trunk_rows(x, rows, block)
    assert out.shape[1] == N
    d = TrunkDims(G, N, C_in, R)
    d_out = d_out.contiguous()
    assert out.is_contiguous() and d_out.shape == out.shape and d_out.dtype == torch.bfloat16
    nb = lib().cat_trunk_backward_blocks(C.byref(d))
    dev = x.device
    pw1 = torch.empty(G, nb, 64, 32, dtype=torch.float32, device=dev)
    pb1 = torch.empty(G, nb, 64, dtype=torch.float32, device=dev)
    pw2 = torch.empty(G, nb, 32, 320, dtype=torch.float32, device=dev)
    pb2 = torch.empty(G, nb, 32, dtype=torch.float32, device=dev)
    a = TrunkBwd(d, _trunk_params(w1, b1, w2, b2, G, C_in), x.data_ptr(), x.stride(0), x.stride(1), xr, out.data_ptr(), d_out.data_ptr(),
                 out.stride(0), out.stride(1), pw1.data_ptr(), pb1.data_ptr(), pw2.data_ptr(), pb2.data_ptr())
    _check(lib().cat_trunk_backward(C.byref(a), _stream()), "cat_trunk_backward")
    return pw1, pb1, pw2, pb2


def trunk_grad_finish(parts, C_in: int, R: int, slots=None):
    """The four slab buffers of ``trunk_backward`` -> the parameter gradients in the parameters' own shapes (bf16): ADDED into
    ``slots`` = (dw1, db1, dw2, db2) views (returns None) or returned as new tensors."""
    import torch
    pw1, pb1, pw2, pb2 = parts
    G, nb = pw2.shape[:2]
    acc = slots is not None
    if not acc:
        dev = pw1.device
        slots = (torch.empty(G, 64, C_in, 5, dtype=torch.bfloat16, device=dev), torch.empty(G, 64, dtype=torch.bfloat16, device=dev),
                 torch.empty(G, 32, 64, 5, dtype=torch.bfloat16, device=dev), torch.empty(G, 32, dtype=torch.bfloat16, device=dev))
    for t in slots:
        assert t.dtype == torch.bfloat16 and t[0].is_contiguous()
    a = TrunkFinish(TrunkDims(G, 16, C_in, R), nb, 1 if acc else 0, pw1.data_ptr(), pb1.data_ptr(), pw2.data_ptr(), pb2.data_ptr(),
                    slots[0].data_ptr(), slots[1].data_ptr(), slots[2].data_ptr(), slots[3].data_ptr(),
                    slots[0].stride(0), slots[1].stride(0), slots[2].stride(0), slots[3].stride(0))
    _check(lib().cat_trunk_grad_finish(C.byref(a), _stream()), "cat_trunk_grad_finish")
    return None if acc else slots


# ---------------------------------------------------------------------------------------------- PPO loss / optimiser step
PPO_CHUNKS = 64


def ppo_loss_grad(logits, values, actions, old_logp, adv, ret, ratio_clip: float, value_scale: float, entropy_scale: float):
    """logits bf16 [G, ..., 4], values bf16 [G, ...(, 1)], actions int64 / old_logp / adv / ret fp32 [G, ...] (M samples per
    agent each, contiguous).  Returns (sums fp32 [G, 4] = surrogate, squared value error, entropy, KL; d_logits; d_values)."""
    import torch
    G = logits.shape[0]
    M = logits[0].numel() // 4
    for t, dt in ((logits, torch.bfloat16), (values, torch.bfloat16), (actions, torch.int64), (old_logp, torch.float32),
                  (adv, torch.float32), (ret, torch.float32)):
        assert t.dtype == dt and t.is_contiguous() and t.shape[0] == G
    assert values[0].numel() == M and actions[0].numel() == M and old_logp[0].numel() == M and adv[0].numel() == M and ret[0].numel() == M
    d_logits, d_values = torch.empty_like(logits), torch.empty_like(values)
    partial = torch.empty(G, PPO_CHUNKS, 4, dtype=torch.float32, device=logits.device)
    a = PpoLoss(G, M, PPO_CHUNKS, 0, logits.data_ptr(), values.data_ptr(), actions.data_ptr(), old_logp.data_ptr(), adv.data_ptr(),
                ret.data_ptr(), ratio_clip, value_scale, entropy_scale, 0.0, d_logits.data_ptr(), d_values.data_ptr(), partial.data_ptr())
    _check(lib().cat_ppo_loss_grad(C.byref(a), _stream()), "cat_ppo_loss_grad")
    return torch.bmm(ones_row(G, PPO_CHUNKS, logits.device), partial).squeeze(1), d_logits, d_values


def ppo_adam_step(ar, col_train, epoch_active, m, v, steps, master, lp, kl_out, scratch, lr, beta1, beta2, eps, grad_norm_clip,
                  kl_threshold) -> None:
    """In-place optimiser step on the flat [G, P] buffers (see include/cat_ppo.h); ``lp`` = bf16 copy or None;
    ``scratch`` fp32 [G, 256]."""
    import torch
    G, P = master.shape
    for t in (ar, col_train, epoch_active, m, v, steps, master, kl_out, scratch):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert ar.shape == (G, P + 1) and col_train.shape == (G, P) and scratch.shape == (G, 256) and kl_out.shape == (G,)
    assert lp is None or (lp.dtype == torch.bfloat16 and lp.is_contiguous() and lp.shape == (G, P))
    a = PpoAdam(G, P, 256, 0, ar.data_ptr(), col_train.data_ptr(), epoch_active.data_ptr(), m.data_ptr(), v.data_ptr(), steps.data_ptr(),
                master.data_ptr(), _ptr(lp), kl_out.data_ptr(), scratch.data_ptr(), lr, beta1, beta2, eps, grad_norm_clip, kl_threshold or 0.0)
    _check(lib().cat_ppo_adam_step(C.byref(a), _stream()), "cat_ppo_adam_step")


# the hyper block of the _dev entries: fp32 [G, PPO_HYPER_STRIDE] on the device (include/cat_ppo.h)
PPO_HYPER_STRIDE = 8                                                    # CAT_PPO_HYPER_STRIDE
HYPER_LR, HYPER_ENTROPY, HYPER_RATIO_CLIP, HYPER_KL_SUM, HYPER_KL_COUNT = range(5)      # CAT_PPO_HYPER_*
SCHED_KL, SCHED_ANNEAL = 1, 2                                           # cat_ppo_schedule.mode (bits)
ANNEAL_LR, ANNEAL_ENTROPY, ANNEAL_RATIO_CLIP = 1, 2, 4                  # cat_ppo_schedule.anneal_mask (bits)
SCHED_MAX_AGENTS = 8                                                    # CAT_ROLLOUT_MAX_AGENTS


def _hyper_ok(hyper, G: int, like) -> None:
    import torch
    assert hyper.dtype == torch.float32 and hyper.is_contiguous() and hyper.shape == (G, PPO_HYPER_STRIDE) and hyper.device == like.device


def ppo_loss_grad_dev(logits, values, actions, old_logp, adv, ret, hyper, value_scale: float):
    """``ppo_loss_grad`` with agent g's ratio clip and entropy scale read from ``hyper`` fp32 [G, 8] on the device (columns HYPER_RATIO_CLIP
    and HYPER_ENTROPY) at the time the kernel runs: a captured call follows the block without a recapture."""
    import torch
    G = logits.shape[0]
    M = logits[0].numel() // 4
    for t, dt in ((logits, torch.bfloat16), (values, torch.bfloat16), (actions, torch.int64), (old_logp, torch.float32),
                  (adv, torch.float32), (ret, torch.float32)):
        assert t.dtype == dt and t.is_contiguous() and t.shape[0] == G
    assert values[0].numel() == M and actions[0].numel() == M and old_logp[0].numel() == M and adv[0].numel() == M and ret[0].numel() == M
    _hyper_ok(hyper, G, logits)
    d_logits, d_values = torch.empty_like(logits), torch.empty_like(values)
    partial = torch.empty(G, PPO_CHUNKS, 4, dtype=torch.float32, device=logits.device)
    a = PpoLossDev(G, M, PPO_CHUNKS, 0, logits.data_ptr(), values.data_ptr(), actions.data_ptr(), old_logp.data_ptr(), adv.data_ptr(),
                   ret.data_ptr(), 0.0, value_scale, 0.0, 0.0, d_logits.data_ptr(), d_values.data_ptr(), partial.data_ptr(), hyper.data_ptr())
    _check(lib().cat_ppo_loss_grad_dev(C.byref(a), _stream()), "cat_ppo_loss_grad_dev")
    return torch.bmm(ones_row(G, PPO_CHUNKS, logits.device), partial).squeeze(1), d_logits, d_values


def ppo_adam_step_dev(ar, col_train, epoch_active, m, v, steps, master, lp, kl_out, scratch, hyper, beta1, beta2, eps, grad_norm_clip,
                      kl_threshold) -> None:
    """``ppo_adam_step`` with agent g's learning rate read from ``hyper`` fp32 [G, 8] on the device (column HYPER_LR); an agent that enters
    the step with ``epoch_active`` set adds its KL to HYPER_KL_SUM and 1 to HYPER_KL_COUNT."""
    import torch
    G, P = master.shape
    for t in (ar, col_train, epoch_active, m, v, steps, master, kl_out, scratch):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert ar.shape == (G, P + 1) and col_train.shape == (G, P) and scratch.shape == (G, 256) and kl_out.shape == (G,)
    assert lp is None or (lp.dtype == torch.bfloat16 and lp.is_contiguous() and lp.shape == (G, P))
    _hyper_ok(hyper, G, master)
    a = PpoAdamDev(G, P, 256, 0, ar.data_ptr(), col_train.data_ptr(), epoch_active.data_ptr(), m.data_ptr(), v.data_ptr(), steps.data_ptr(),
                   master.data_ptr(), _ptr(lp), kl_out.data_ptr(), scratch.data_ptr(), 0.0, beta1, beta2, eps, grad_norm_clip,
                   kl_threshold or 0.0, hyper.data_ptr())
    _check(lib().cat_ppo_adam_step_dev(C.byref(a), _stream()), "cat_ppo_adam_step_dev")


def ppo_schedule_step(hyper, sched_active, mode: int, *, kl_target: float = 0.008, kl_factor: float = 2.0, lr_factor: float = 1.5,
                      lr_min: float = 1e-6, lr_max: float = 1e-2, anneal_mask: int = 0, progress: float = 0.0,
                      lr=(0.0, 0.0), entropy=(0.0, 0.0), ratio_clip=(0.0, 0.0)) -> None:
    """The schedule rule on ``hyper`` fp32 [G, 8] in place (one tiny launch; include/cat_ppo.h): ``mode`` = SCHED_ANNEAL (the fields of
    ``anneal_mask`` <- x0 + (x1 - x0) * progress from the (x0, x1) pairs), SCHED_KL (the KL-adaptive learning rate of the agents with
    ``sched_active`` fp32 [G] set, from the epoch's KL sum, which is cleared) or both (the anneal first)."""
    import torch
    G = hyper.shape[0]
    assert 1 <= G <= SCHED_MAX_AGENTS
    _hyper_ok(hyper, G, hyper)
    assert sched_active.dtype == torch.float32 and sched_active.is_contiguous() and sched_active.shape == (G,) and sched_active.device == hyper.device
    a = PpoSchedule(G, mode, anneal_mask, 0, hyper.data_ptr(), sched_active.data_ptr(), kl_target, kl_factor, lr_factor, lr_min, lr_max,
                    progress, lr[0], lr[1], entropy[0], entropy[1], ratio_clip[0], ratio_clip[1])
    _check(lib().cat_ppo_schedule_step(C.byref(a), _stream()), "cat_ppo_schedule_step")


class PpoGae(C.Structure):
    _fields_ = [("G", C.c_int32), ("T", C.c_int32), ("N", C.c_int32), ("pad", C.c_int32), ("rewards", C.c_void_p), ("values", C.c_void_p),
                ("dones", C.c_void_p), ("last_values", C.c_void_p), ("gamma", C.c_float), ("lambda_", C.c_float),
                ("adv", C.c_void_p), ("ret", C.c_void_p)]


def ppo_gae(rewards, values, dones, last_values, gamma: float, lam: float, adv_out, ret_out) -> None:
    """rewards, values, adv_out, ret_out fp32 [G, T, N] contiguous; dones bool / uint8 [T, N]; last_values fp32 [G, N]: the whole
    reverse scan in one launch (include/cat_ppo.h)."""
    import torch
    G, T, N = rewards.shape
    for t in (rewards, values, adv_out, ret_out):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (G, T, N)
    last_values = last_values.contiguous()
    assert last_values.dtype == torch.float32 and last_values.shape == (G, N)
    d8 = dones.contiguous().view(torch.uint8) if dones.dtype == torch.bool else dones.contiguous()
    assert d8.dtype == torch.uint8 and d8.shape == (T, N)
    a = PpoGae(G, T, N, 0, rewards.data_ptr(), values.data_ptr(), d8.data_ptr(), last_values.data_ptr(), gamma, lam,
               adv_out.data_ptr(), ret_out.data_ptr())
    _check(lib().cat_ppo_gae_scan(C.byref(a), _stream()), "cat_ppo_gae_scan")


class PpoGaeScaled(C.Structure):
    _fields_ = PpoGae._fields_ + [("scale", C.c_void_p)]


def ppo_gae_scaled(rewards, values, dones, last_values, scale, gamma: float, lam: float, adv_out, ret_out) -> None:
    """``ppo_gae`` over a critic trained on normalised returns: ``scale`` fp32 [G, 2] = (mu, sigma) on the device; values and last_values
    are denormalised (v * sigma, then + mu) as they are read, ret_out is the raw return (include/cat_ppo.h)."""
    import torch
    G, T, N = rewards.shape
    for t in (rewards, values, adv_out, ret_out):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (G, T, N)
    last_values = last_values.contiguous()
    assert last_values.dtype == torch.float32 and last_values.shape == (G, N)
    assert scale.dtype == torch.float32 and scale.shape == (G, 2) and scale.is_contiguous() and scale.device == rewards.device
    d8 = dones.contiguous().view(torch.uint8) if dones.dtype == torch.bool else dones.contiguous()
    assert d8.dtype == torch.uint8 and d8.shape == (T, N)
    a = PpoGaeScaled(G, T, N, 0, rewards.data_ptr(), values.data_ptr(), d8.data_ptr(), last_values.data_ptr(), gamma, lam,
                     adv_out.data_ptr(), ret_out.data_ptr(), scale.data_ptr())
    _check(lib().cat_ppo_gae_scan_scaled(C.byref(a), _stream()), "cat_ppo_gae_scan_scaled")


PPO_MOMENT_CHUNK = 4096         # CAT_PPO_MOMENT_CHUNK


class PpoMoments(C.Structure):
    _fields_ = [("G", C.c_int32), ("M", C.c_int32), ("x", C.c_void_p), ("partial", C.c_void_p), ("batch_out", C.c_void_p),
                ("state", C.c_void_p), ("scale_out", C.c_void_p)]


def ppo_moment_chunks(M: int) -> int:
    """Rows of the scratch buffer ``ppo_moments`` needs per agent for M samples: ceil(M / 4096)."""
    return lib().cat_ppo_moment_chunks(M)


def ppo_moments(x, state=None, scale_out=None, batch_out=None, partial=None):
    """x fp32 [G, M] contiguous: the f64 moments (n, mean, M2) of every row in the fixed order of include/cat_ppo.h.  ``batch_out`` f64
    [G, 3] receives them; ``state`` f64 [G, 3] is merged with them in place; ``scale_out`` fp32 [G, 2] receives (mu, sigma) of the merged
    state (needs ``state``).  ``partial``: f64 [G, chunks, 3] scratch (allocated when None; pass one for a captured call).  Two
    launches on the current stream.  Returns ``partial``."""
    import torch
    assert x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous()
    G, M = x.shape
    if scale_out is not None and state is None:
        raise ValueError("ppo_moments: scale_out needs state")
    chunks = ppo_moment_chunks(M)
    if partial is None:
        partial = torch.empty(G, chunks, 3, dtype=torch.float64, device=x.device)
    assert partial.dtype == torch.float64 and partial.is_contiguous() and partial.shape == (G, chunks, 3) and partial.device == x.device
    for t, dt, shape in ((state, torch.float64, (G, 3)), (batch_out, torch.float64, (G, 3)), (scale_out, torch.float32, (G, 2))):
        assert t is None or (t.dtype == dt and t.shape == shape and t.is_contiguous() and t.device == x.device)
    a = PpoMoments(G, M, x.data_ptr(), partial.data_ptr(), _ptr(batch_out), _ptr(state), _ptr(scale_out))
    _check(lib().cat_ppo_moments(C.byref(a), _stream()), "cat_ppo_moments")
    return partial


# ---------------------------------------------------------------------------------------------- dense-layer epilogues
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
DENSE_CHUNKS = 64


class DenseDims(C.Structure):
    _fields_ = [("G", C.c_int32), ("M", C.c_int32), ("out", C.c_int32), ("act", C.c_int32)]


def dense_bias_act_(y, bias, act: int):
    """y bf16 [G, M, out] contiguous <- act(y + bias[g]) in place; bias bf16 [G, out] (row stride free)."""
    import torch
    G, M, out = y.shape
    assert y.dtype == torch.bfloat16 and y.is_contiguous() and bias.shape == (G, out) and bias.dtype == torch.bfloat16 and bias.stride(1) == 1
    d = DenseDims(G, M, out, act)
    _check(lib().cat_dense_bias_act(C.byref(d), y.data_ptr(), bias.data_ptr(), bias.stride(0), _stream()), "cat_dense_bias_act")
    return y


def dense_act_grad(d_y, y, act: int):
    """(d_y * act'(y), fp32 per-chunk column sums [G, chunks, out] of it: ``sum_chunks`` adds them up).  With ACT_NONE the
    first result is d_y itself."""
    import torch
    G, M, out = d_y.shape
    d_y = d_y.contiguous()
    assert d_y.dtype == torch.bfloat16 and (act == ACT_NONE or (y.shape == d_y.shape and y.is_contiguous()))
    g_out = torch.empty_like(d_y) if act != ACT_NONE else None
    chunks = max(1, min(256, M // 32))
    partial = torch.empty(G, chunks, out, dtype=torch.float32, device=d_y.device)
    d = DenseDims(G, M, out, act)
    _check(lib().cat_dense_act_grad(C.byref(d), d_y.data_ptr(), _ptr(y) if act != ACT_NONE else 0, _ptr(g_out), partial.data_ptr(), chunks,
                                    _stream()), "cat_dense_act_grad")
    return (g_out if g_out is not None else d_y), partial


def sum_chunks(partial, dst=None, dst2=None, accumulate: bool = False):
    """partial fp32 [G, chunks, ...] -> bf16 [G, ...] sums over the chunks: into ``dst`` (and ``dst2``), each [G, n] with
    contiguous rows and any row stride, optionally added to what they hold; a new tensor when ``dst`` is None."""
    import torch
    G, chunks = partial.shape[:2]
    n = partial[0, 0].numel()
    assert partial.dtype == torch.float32 and partial.is_contiguous()
    if dst is None:
        dst = torch.empty((G,) + tuple(partial.shape[2:]), dtype=torch.bfloat16, device=partial.device)
    for t in (dst, dst2):
        assert t is None or (t.dtype == torch.bfloat16 and t.shape[0] == G and t[0].numel() == n and t[0].is_contiguous())
    _check(lib().cat_dense_sum_chunks(partial.data_ptr(), G, chunks, n, dst.data_ptr(), dst.stride(0), _ptr(dst2),
                                      0 if dst2 is None else dst2.stride(0), 1 if accumulate else 0, _stream()), "cat_dense_sum_chunks")
    return dst


class WgradArgs(C.Structure):
    _fields_ = [("G", C.c_int32), ("K", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("a", C.c_void_p), ("b", C.c_void_p),
                ("partial", C.c_void_p), ("splits", C.c_int32), ("pad", C.c_int32),
                ("b1", C.c_void_p), ("partial1", C.c_void_p), ("N1", C.c_int32), ("pad1", C.c_int32)]


def wgrad_supported(g, x) -> bool:
    return g.shape[1] >= 512


class SumJob(C.Structure):
    _fields_ = [("partial", C.c_void_p), ("chunks", C.c_int32), ("n", C.c_int32), ("dst0", C.c_void_p), ("sd0_g", C.c_int64),
                ("dst1", C.c_void_p), ("sd1_g", C.c_int64), ("accumulate", C.c_int32), ("pad", C.c_int32)]


def _sum_job(partial, dst, accumulate: bool) -> SumJob:
    G, chunks = partial.shape[:2]
    n = partial[0, 0].numel()
    assert partial.is_contiguous() and dst.shape[0] == G and dst[0].numel() == n and dst[0].is_contiguous()
    return SumJob(partial.data_ptr(), chunks, n, dst.data_ptr(), dst.stride(0), 0, 0, 1 if accumulate else 0, 0)


def dense_wgrad(g, x, slot=None, bias_job=None):
    """g bf16 [G, K, M] (gradient of a layer's pre-activations), x bf16 [G, K, N] (its input) -> sum_k g[k, m] x[k, n] as
    bf16 [G, M, N]: ADDED into ``slot`` (a [G, M, N] view whose [M, N] blocks are contiguous) when given, else returned.
    ``bias_job`` = (partial fp32 [G, chunks, M], bias slot [G, M]): that chunk sum rides in the same launch."""
    import torch
    G, K, M = g.shape
    N = x.shape[2]
    g, x = g.contiguous(), x.contiguous()
    assert g.dtype == x.dtype == torch.bfloat16 and x.shape[:2] == (G, K)
    S = lib().cat_dense_wgrad_splits(G, K, M, N)
    partial = torch.empty(G, S, M * N, dtype=torch.float32, device=g.device)
    a = WgradArgs(G, K, M, N, g.data_ptr(), x.data_ptr(), partial.data_ptr(), S, 0, None, None, 0, 0)
    _check(lib().cat_dense_wgrad(C.byref(a), _stream()), "cat_dense_wgrad")
    out = None
    if slot is not None:
        assert slot.shape == (G, M, N) and slot[0].is_contiguous()
        dst = slot.view(G, M * N) if slot.is_contiguous() else slot.as_strided((G, M * N), (slot.stride(0), 1))
    else:
        out = torch.empty(G, M * N, dtype=torch.bfloat16, device=g.device)
        dst = out
    ja = _sum_job(partial, dst, slot is not None)
    jb = None if bias_job is None else _sum_job(bias_job[0], bias_job[1], True)
    _check(lib().cat_dense_sum_chunks2(C.byref(ja), None if jb is None else C.byref(jb), G, _stream()), "cat_dense_sum_chunks2")
    return None if slot is not None else out.view(G, M, N)


def dense_wgrad2(g, x0, x1, slot0, slot1) -> None:
    """The weight gradients of TWO layers that share the gradient g [G, K, M] of their summed pre-activations (an LSTM layer:
    W_ih with its input x0 [G, K, N0], W_hh with h_in x1 [G, K, N1]): one launch reads g once, one launch adds the slabs of
    both up into ``slot0`` [G, M, N0] and ``slot1`` [G, M, N1]."""
    import torch
    G, K, M = g.shape
    N0, N1 = x0.shape[2], x1.shape[2]
    g, x0, x1 = g.contiguous(), x0.contiguous(), x1.contiguous()
    assert g.dtype == x0.dtype == x1.dtype == torch.bfloat16 and x0.shape[:2] == (G, K) and x1.shape[:2] == (G, K)
    S = lib().cat_dense_wgrad_splits(G, K, M, 128 * (-(-N0 // 128) - (-N1 // 128)))
    p0 = torch.empty(G, S, M * N0, dtype=torch.float32, device=g.device)
    p1 = torch.empty(G, S, M * N1, dtype=torch.float32, device=g.device)
    a = WgradArgs(G, K, M, N0, g.data_ptr(), x0.data_ptr(), p0.data_ptr(), S, 0, x1.data_ptr(), p1.data_ptr(), N1, 0)
    _check(lib().cat_dense_wgrad(C.byref(a), _stream()), "cat_dense_wgrad")
    jobs = []
    for part, slot, N in ((p0, slot0, N0), (p1, slot1, N1)):
        assert slot.shape == (G, M, N) and slot[0].is_contiguous()
        dst = slot.view(G, M * N) if slot.is_contiguous() else slot.as_strided((G, M * N), (slot.stride(0), 1))
        jobs.append(_sum_job(part, dst, True))
    _check(lib().cat_dense_sum_chunks2(C.byref(jobs[0]), C.byref(jobs[1]), G, _stream()), "cat_dense_sum_chunks2")


class GemmArgs(C.Structure):
    _fields_ = [("G", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("x_or_gr", C.c_void_p), ("w", C.c_void_p),
                ("sw_g", C.c_int64), ("bias", C.c_void_p), ("sb_g", C.c_int64), ("act", C.c_int32), ("pad", C.c_int32), ("out", C.c_void_p)]


def gemm_supported(x, w) -> bool:
    """The layer kernels take rows of 16-byte runs: in-features a multiple of 8, weight rows contiguous and aligned."""
    return (x.shape[2] % 8 == 0 and w.stride(2) == 1 and w.stride(1) == w.shape[2] and w.stride(0) % 8 == 0 and w.data_ptr() % 16 == 0)


def dense_forward(x, w, bias, act: int):
    """act(x [G, M, K] @ w [G, N, K]^T + bias [G, N]) -> bf16 [G, M, N]; bias may be None (act must then be ACT_NONE)."""
    import torch
    G, M, K = x.shape
    N = w.shape[1]
    x = x.contiguous()
    assert x.dtype == w.dtype == torch.bfloat16 and w.shape == (G, N, K) and gemm_supported(x, w)
    assert bias is None or (bias.shape == (G, N) and bias.dtype == torch.bfloat16 and bias.stride(1) == 1)
    y = torch.empty(G, M, N, dtype=torch.bfloat16, device=x.device)
    a = GemmArgs(G, M, N, K, x.data_ptr(), w.data_ptr(), w.stride(0), _ptr(bias), 0 if bias is None else bias.stride(0), act, 0, y.data_ptr())
    _check(lib().cat_dense_forward(C.byref(a), _stream()), "cat_dense_forward")
    return y


def dense_dgrad(gr, w):
    """gr [G, M, N] @ w [G, N, K] -> bf16 [G, M, K]: the gradient w.r.t. the layer's input."""
    import torch
    G, M, N = gr.shape
    K = w.shape[2]
    gr = gr.contiguous()
    assert gr.dtype == w.dtype == torch.bfloat16 and w.shape == (G, N, K) and w.stride(2) == 1 and w.stride(1) == K and K % 8 == 0
    dx = torch.empty(G, M, K, dtype=torch.bfloat16, device=gr.device)
    a = GemmArgs(G, M, N, K, gr.data_ptr(), w.data_ptr(), w.stride(0), 0, 0, 0, 0, dx.data_ptr())
    _check(lib().cat_dense_dgrad(C.byref(a), _stream()), "cat_dense_dgrad")
    return dx


_ONES = {}


def ones_row(G: int, n: int, device):
    """cached fp32 [G, 1, n] of ones (the left operand of the "add the slabs up" GEMMs)"""
    import torch
    key = (G, n, str(device))
    if key not in _ONES:
        _ONES[key] = torch.ones(G, 1, n, dtype=torch.float32, device=device)
    return _ONES[key]


# ---------------------------------------------------------------------------------------------- rollout tick glue
class PackArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("A", C.c_int32), ("R", C.c_int32), ("G", C.c_int32), ("agent", C.c_int32 * 8),
                ("n_cops", C.c_int32), ("first_agent_state", C.c_int32), ("distance_scale", C.c_float), ("type_scale", C.c_float),
                ("obs_distance", C.c_void_p), ("obs_type", C.c_void_p), ("shared_distance", C.c_void_p), ("shared_type", C.c_void_p),
                ("policy_in", C.c_void_p), ("sp_g", C.c_int64), ("sp_n", C.c_int64),
                ("value_in", C.c_void_p), ("sv_g", C.c_int64), ("sv_n", C.c_int64)]


class SampleArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("A", C.c_int32), ("G", C.c_int32), ("pad", C.c_int32), ("agent", C.c_int32 * 8),
                ("logits", C.c_void_p), ("uniform", C.c_void_p), ("values", C.c_void_p),
                ("act_out", C.c_void_p), ("logp_out", C.c_void_p), ("value_out", C.c_void_p), ("sa_g", C.c_int64), ("sl_g", C.c_int64),
                ("actions", C.c_void_p)]


def rollout_pack(raw, agent_indices, n_cops: int, first_agent_state: bool, distance_scale: float, type_scale: float, policy_in, value_in):
    """raw = the env core's output buffers (``VecCopsEnv.raw_outputs()``) -> policy_in bf16 [G, N, 2R], value_in bf16
    [G, N, 4R] (views with contiguous rows and any outer strides)."""
    import torch
    od, ot, sd, st = raw["obs_distance"], raw["obs_type"], raw["shared_distance"], raw["shared_type"]
    N, A, R = od.shape
    G = len(agent_indices)
    assert od.dtype == torch.float16 and ot.dtype == torch.uint8 and all(t.is_contiguous() for t in (od, ot, sd, st))
    for t, w in ((policy_in, 2 * R), (value_in, 4 * R)):
        assert t.dtype == torch.bfloat16 and t.shape == (G, N, w) and t.stride(2) == 1
    a = PackArgs(N, A, R, G, (C.c_int32 * 8)(*agent_indices), n_cops, 1 if first_agent_state else 0, distance_scale, type_scale,
                 od.data_ptr(), ot.data_ptr(), sd.data_ptr(), st.data_ptr(), policy_in.data_ptr(), policy_in.stride(0), policy_in.stride(1),
                 value_in.data_ptr(), value_in.stride(0), value_in.stride(1))
    _check(lib().cat_rollout_pack(C.byref(a), _stream()), "cat_rollout_pack")


def rollout_sample(logits, uniform, values, act_out, logp_out, value_out, actions, agent_indices) -> None:
    """logits bf16 [G, N, 4]; uniform fp32 [G, N]; values bf16 [G, N] or None; act_out int64 / logp_out, value_out fp32
    [G, N] row-strided views; actions int32 [N, A]: column ``agent_indices[g]`` receives agent g's draw."""
    import torch
    G, N, _ = logits.shape
    assert logits.dtype == torch.bfloat16 and logits.is_contiguous() and uniform.dtype == torch.float32 and uniform.is_contiguous()
    assert act_out.dtype == torch.int64 and act_out.stride(1) == 1 and logp_out.dtype == torch.float32 and logp_out.stride(1) == 1
    assert actions.dtype == torch.int32 and actions.is_contiguous() and actions.shape[0] == N
    if value_out is not None:
        assert values.dtype == torch.bfloat16 and values.is_contiguous() and value_out.stride(0) == logp_out.stride(0) and value_out.stride(1) == 1
    a = SampleArgs(N, actions.shape[1], G, 0, (C.c_int32 * 8)(*agent_indices), logits.data_ptr(), uniform.data_ptr(), _ptr(values),
                   act_out.data_ptr(), logp_out.data_ptr(), _ptr(value_out), act_out.stride(0), logp_out.stride(0), actions.data_ptr())
    _check(lib().cat_rollout_sample(C.byref(a), _stream()), "cat_rollout_sample")


class PostArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("A", C.c_int32), ("G", C.c_int32), ("pad", C.c_int32), ("agent", C.c_int32 * 8),
                ("reward", C.c_void_p), ("terminated", C.c_void_p), ("reward_out", C.c_void_p), ("sr_g", C.c_int64),
                ("done_out", C.c_void_p), ("start_out", C.c_void_p), ("keep_out", C.c_void_p)]


def rollout_post(raw, agent_indices, reward_out, done_out=None, start_out=None, keep_out=None) -> None:
    """raw["reward"] fp32 [N, A], raw["terminated"] u8 [N] -> reward_out fp32 [G, N] (row-strided view); done_out / start_out
    bool [N]; keep_out fp32 [N] = 1 - terminated."""
    import torch
    rew, term = raw["reward"], raw["terminated"]
    N, A = rew.shape
    assert rew.dtype == torch.float32 and rew.is_contiguous() and term.dtype == torch.uint8 and term.shape == (N,)
    assert reward_out.dtype == torch.float32 and reward_out.shape == (len(agent_indices), N) and reward_out.stride(1) == 1
    for t, dt in ((done_out, torch.bool), (start_out, torch.bool), (keep_out, torch.float32)):
        assert t is None or (t.dtype == dt and t.numel() == N and t.is_contiguous())
    a = PostArgs(N, A, len(agent_indices), 0, (C.c_int32 * 8)(*agent_indices), rew.data_ptr(), term.data_ptr(), reward_out.data_ptr(),
                 reward_out.stride(0), _ptr(done_out), _ptr(start_out), _ptr(keep_out))
    _check(lib().cat_rollout_post(C.byref(a), _stream()), "cat_rollout_post")


# ---------------------------------------------------------------------------------------------- episode accounting
EPISODES_STATE_FIELDS = ("ret_run", "len_run", "finished", "cop_wins", "thief_wins", "timeouts", "len_sum", "len_min", "len_max",
                         "ret_sum", "ret_sq", "len_hist")


class EpisodesState(C.Structure):
    """include/cat_episodes.h cat_episodes_state (device pointers)."""
    _fields_ = [(n, C.c_void_p) for n in EPISODES_STATE_FIELDS]


class EpisodesUpdate(C.Structure):
    _fields_ = [("T", C.c_int32), ("N", C.c_int32), ("A", C.c_int32), ("max_step_count", C.c_int32),
                ("reward", C.c_void_p), ("terminated", C.c_void_p), ("truncated", C.c_void_p), ("winner", C.c_void_p),
                ("quota", C.c_void_p), ("s", EpisodesState)]


class EpisodeWindows(C.Structure):
    """include/cat_episodes.h cat_episode_windows_args."""
    _fields_ = [("u", EpisodesUpdate), ("ticks", C.c_void_p)]


class EpisodesSummaryBlock(C.Structure):
    _fields_ = [("episodes", C.c_int64), ("cop_wins", C.c_int64), ("thief_wins", C.c_int64), ("timeouts", C.c_int64),
                ("open_slots", C.c_int64), ("len_sum", C.c_int64), ("len_min", C.c_int32), ("len_max", C.c_int32),
                ("ret_sum", C.c_double * EPISODES_MAX_AGENTS), ("ret_sq", C.c_double * EPISODES_MAX_AGENTS)]


class EpisodesSummary(C.Structure):
    _fields_ = [("N", C.c_int32), ("A", C.c_int32), ("quota", C.c_void_p), ("s", EpisodesState), ("out", C.c_void_p)]


def _episodes_state(state) -> EpisodesState:
    return EpisodesState(*[state[n].data_ptr() for n in EPISODES_STATE_FIELDS])


def episodes_update(state, reward, terminated, truncated, winner, quota, max_step_count: int, ticks=None) -> None:
    """``state``: the tracker's device tensors by name (``EPISODES_STATE_FIELDS``); reward fp32 [T, N, A], terminated / truncated
    u8 [T, N], winner i8 [T, N], all contiguous; quota int32 [N] or None.  One launch on the current stream (capturable).
    ``ticks`` int32 [T, N]: the env ticks each row stands for (``cat_episode_windows_update``); None: one each."""
    import torch
    T, N, A = reward.shape
    assert reward.dtype == torch.float32 and reward.is_contiguous()
    for t, dt in ((terminated, torch.uint8), (truncated, torch.uint8), (winner, torch.int8)):
        assert t.dtype == dt and t.shape == (T, N) and t.is_contiguous()
    assert quota is None or (quota.dtype == torch.int32 and quota.shape == (N,) and quota.is_contiguous())
    assert state["ret_run"].shape == (N, A) and state["len_run"].shape == (N,)
    a = EpisodesUpdate(T, N, A, int(max_step_count), reward.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), winner.data_ptr(),
                       _ptr(quota), _episodes_state(state))
    if ticks is None:
        _check(lib().cat_episodes_update(C.byref(a), _stream()), "cat_episodes_update")
        return
    assert ticks.dtype == torch.int32 and ticks.shape == (T, N) and ticks.is_contiguous() and ticks.device == reward.device
    w = EpisodeWindows(a, ticks.data_ptr())
    _check(lib().cat_episode_windows_update(C.byref(w), _stream()), "cat_episode_windows_update")


def episodes_summary(state, quota, block) -> None:
    """The per-slot ``state`` -> ``block`` (uint8 device tensor of at least ``sizeof(EpisodesSummaryBlock)`` bytes, 8-byte
    aligned).  One launch on the current stream; the caller copies the block to the host."""
    import torch
    N, A = state["ret_run"].shape
    assert block.dtype == torch.uint8 and block.is_contiguous() and block.numel() >= C.sizeof(EpisodesSummaryBlock) and block.data_ptr() % 8 == 0
    a = EpisodesSummary(N, A, _ptr(quota), _episodes_state(state), block.data_ptr())
    _check(lib().cat_episodes_summary(C.byref(a), _stream()), "cat_episodes_summary")


class EpisodesSegmentSummary(C.Structure):
    """include/cat_episodes.h cat_episodes_segment_summary_args."""
    _fields_ = [("N", C.c_int32), ("A", C.c_int32), ("S", C.c_int32), ("seg_start", C.c_int32 * (EPISODES_MAX_SEGMENTS + 1)),
                ("quota", C.c_void_p), ("s", EpisodesState), ("out", C.c_void_p)]


def _check_bounds(N: int, start, max_segments: int) -> None:
    """The rules of the C entries' ``seg_start`` for S + 1 ints: 1 <= S <= max_segments, 0 first, N last, strictly increasing."""
    S = len(start) - 1
    if not 1 <= S <= max_segments:
        raise ValueError(f"{S} segments: 1..{max_segments} are allowed")
    if start[0] != 0 or start[-1] != N:
        raise ValueError(f"the segments must begin at row 0 and end at row {N}: {start}")
    if any(b <= a for a, b in zip(start, start[1:])):
        raise ValueError(f"the segment bounds must be strictly increasing: {start}")


def segment_bounds(N: int, bounds):
    """``bounds``: S + 1 row bounds of S contiguous segments of N slots, checked by the rules of ``cat_act_league_args`` (0 first, N last,
    strictly increasing, 1 <= S <= EPISODES_MAX_SEGMENTS) -> a list of ints.  Raises ValueError."""
    try:
        start = [int(v) for v in bounds]
        exact = all(float(v) == i for v, i in zip(bounds, start))
    except (TypeError, ValueError) as exc:
        raise ValueError(f"segment bounds must be a sequence of integers: {bounds!r}") from exc
    if not exact:
        raise ValueError(f"segment bounds must be integers: {list(bounds)}")
    _check_bounds(N, start, EPISODES_MAX_SEGMENTS)
    return start


def episodes_segment_summary(state, quota, bounds, out) -> None:
    """The per-slot ``state`` -> one ``EpisodesSummaryBlock`` per segment in ``out`` (uint8 device tensor of at least S blocks, 8-byte
    aligned; bytes beyond block S - 1 are not touched).  ``bounds``: see ``segment_bounds`` (ValueError before the library is touched).
    One launch of S workgroups on the current stream (capturable); the caller copies the blocks to the host."""
    import torch
    N, A = state["ret_run"].shape
    start = segment_bounds(N, bounds)
    S = len(start) - 1
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= S * C.sizeof(EpisodesSummaryBlock)
            and out.data_ptr() % 8 == 0):
        raise ValueError(f"out must be a contiguous, 8-byte aligned uint8 tensor of at least {S} x {C.sizeof(EpisodesSummaryBlock)} bytes")
    a = EpisodesSegmentSummary(N, A, S, (C.c_int32 * (EPISODES_MAX_SEGMENTS + 1))(*start), _ptr(quota), _episodes_state(state), out.data_ptr())
    _check(lib().cat_episodes_segment_summary(C.byref(a), _stream()), "cat_episodes_segment_summary")


# ---------------------------------------------------------------------------------------------- position statistics
POSITIONS_OCC, POSITIONS_SEEN, POSITIONS_SPAWN = 0, 1, 2      # CAT_POSITIONS_*: the planes of ``counts``
POSITIONS_MAX_TICKS = 65536                                    # CAT_POSITIONS_MAX_TICKS: rows of one launch


class PositionsArgs(C.Structure):
    """include/cat_render.h cat_render_positions_args."""
    _fields_ = [("T", C.c_int32), ("N", C.c_int32), ("A", C.c_int32), ("n_cops", C.c_int32),
                ("R", C.c_int32), ("cell", C.c_int32), ("Wc", C.c_int32), ("Hc", C.c_int32), ("G", C.c_int32), ("pad", C.c_int32),
                ("team_positions", C.c_void_p), ("terminated", C.c_void_p), ("obs_type", C.c_void_p), ("group", C.c_void_p),
                ("quota", C.c_void_p), ("counts", C.c_void_p), ("outside", C.c_void_p), ("rows", C.c_void_p), ("done", C.c_void_p)]


def positions_update(team_positions, terminated, obs_type, group, quota, counts, outside, rows, done, n_cops: int, cell: int) -> PositionsArgs:
    """team_positions f16 [T, N, A, 2], terminated u8 [T, N], obs_type u8 [T, N, A, R] or None, all contiguous; group / quota int32 [N]
    or None; counts int64 [G, 3, A, Wc, Hc], outside int64 [G, A], rows int64 [G], done int32 [N] (``positions.PositionTracker`` owns
    them).  One launch on the current stream (capturable); T <= POSITIONS_MAX_TICKS.  Returns the checked argument block: while every
    buffer stays where it is, ``positions_launch`` repeats the launch without the checks."""
    import torch
    T, N, A, _ = team_positions.shape
    G, _, _, Wc, Hc = counts.shape
    assert team_positions.dtype == torch.float16 and team_positions.shape == (T, N, A, 2) and team_positions.is_contiguous()
    assert terminated.dtype == torch.uint8 and terminated.shape == (T, N) and terminated.is_contiguous()
    R = 0
    if obs_type is not None:
        R = obs_type.shape[3]
        assert obs_type.dtype == torch.uint8 and obs_type.shape == (T, N, A, R) and obs_type.is_contiguous()
    for t in (group, quota):
        assert t is None or (t.dtype == torch.int32 and t.shape == (N,) and t.is_contiguous())
    assert counts.dtype == torch.int64 and counts.shape == (G, 3, A, Wc, Hc) and counts.is_contiguous()
    assert outside.dtype == torch.int64 and outside.shape == (G, A) and outside.is_contiguous()
    assert rows.dtype == torch.int64 and rows.shape == (G,) and done.dtype == torch.int32 and done.shape == (N,)
    dev = counts.device
    assert all(t is None or t.device == dev for t in (team_positions, terminated, obs_type, group, quota, outside, rows, done))
    a = PositionsArgs(T, N, A, int(n_cops), R, int(cell), Wc, Hc, G, 0, team_positions.data_ptr(), terminated.data_ptr(), _ptr(obs_type),
                      _ptr(group), _ptr(quota), counts.data_ptr(), outside.data_ptr(), rows.data_ptr(), done.data_ptr())
    positions_launch(a)
    return a


def positions_launch(a: PositionsArgs) -> None:
    """One launch of ``cat_render_positions_update`` with an argument block ``positions_update`` has checked."""
    _check(lib().cat_render_positions_update(C.byref(a), _stream()), "cat_render_positions_update")


POSITIONS_CAPTURE, POSITIONS_TIMEOUT = 0, 1                   # CAT_POSITIONS_*: the planes of ``ends``


class PositionsEndsArgs(C.Structure):
    """include/cat_render.h cat_render_positions_ends_args."""
    _fields_ = [("T", C.c_int32), ("N", C.c_int32), ("A", C.c_int32), ("cell", C.c_int32),
                ("Wc", C.c_int32), ("Hc", C.c_int32), ("G", C.c_int32), ("pad", C.c_int32),
                ("final_positions", C.c_void_p), ("terminated", C.c_void_p), ("truncated", C.c_void_p), ("group", C.c_void_p),
                ("quota", C.c_void_p), ("done_before", C.c_void_p), ("ends", C.c_void_p), ("ends_outside", C.c_void_p)]


def positions_ends_update(final_positions, terminated, truncated, group, quota, done_before, ends, ends_outside, cell: int) -> PositionsEndsArgs:
    """final_positions f16 [T, N, A, 2], terminated / truncated u8 [T, N], all contiguous; group / quota / done_before int32 [N] or None;
    ends int64 [G, 2, A, Wc, Hc], ends_outside int64 [G, 2, A].  One launch of ``cat_render_positions_ends_update`` on the current stream
    (capturable); T <= POSITIONS_MAX_TICKS.  ``done_before`` is read, not written: launch this BEFORE the ``positions_update`` of the same rows
    advances it.  Returns the checked argument block for ``positions_ends_launch``."""
    import torch
    T, N, A, _ = final_positions.shape
    G, _, _, Wc, Hc = ends.shape
    assert final_positions.dtype == torch.float16 and final_positions.shape == (T, N, A, 2) and final_positions.is_contiguous()
    for t in (terminated, truncated):
        assert t.dtype == torch.uint8 and t.shape == (T, N) and t.is_contiguous()
    for t in (group, quota, done_before):
        assert t is None or (t.dtype == torch.int32 and t.shape == (N,) and t.is_contiguous())
    assert ends.dtype == torch.int64 and ends.shape == (G, 2, A, Wc, Hc) and ends.is_contiguous()
    assert ends_outside.dtype == torch.int64 and ends_outside.shape == (G, 2, A) and ends_outside.is_contiguous()
    dev = ends.device
    assert all(t is None or t.device == dev for t in (final_positions, terminated, truncated, group, quota, done_before, ends_outside))
    a = PositionsEndsArgs(T, N, A, int(cell), Wc, Hc, G, 0, final_positions.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), _ptr(group),
                          _ptr(quota), _ptr(done_before), ends.data_ptr(), ends_outside.data_ptr())
    positions_ends_launch(a)
    return a


def positions_ends_launch(a: PositionsEndsArgs) -> None:
    """One launch of ``cat_render_positions_ends_update`` with an argument block ``positions_ends_update`` has checked."""
    _check(lib().cat_render_positions_ends_update(C.byref(a), _stream()), "cat_render_positions_ends_update")


# ---------------------------------------------------------------------------------------------- navigation (pursue / flee)
NAV_MAX_CELLS, NAV_MAX_MAPS, NAV_NONE = 4096, 16, 0xFFFF        # CAT_NAV_MAX_CELLS / _MAX_MAPS / _NONE
NAV_MAX_NAVIGATORS, NAV_MAX_SEGMENTS = 8, 32                    # CAT_NAV_MAX_NAVIGATORS / _MAX_SEGMENTS
NAV_PURSUE, NAV_FLEE = 0, 1                                     # CAT_NAV_PURSUE / CAT_NAV_FLEE; -1: leaves the column alone


class NavBuildArgs(C.Structure):
    """include/cat_render.h cat_render_nav_build_args."""
    _fields_ = [("n_maps", C.c_int32), ("pad", C.c_int32), ("grid_host", C.c_void_p), ("grid", C.c_void_p), ("free", C.c_void_p), ("hops", C.c_void_p)]


class NavStepArgs(C.Structure):
    """include/cat_render.h cat_render_nav_step_args."""
    _fields_ = [("N", C.c_int32), ("A", C.c_int32), ("G", C.c_int32), ("S", C.c_int32), ("n_maps", C.c_int32), ("cell", C.c_int32),
                ("agent", C.c_int32 * NAV_MAX_NAVIGATORS), ("opp_mask", C.c_uint32 * NAV_MAX_NAVIGATORS),
                ("seg_start", C.c_int32 * (NAV_MAX_SEGMENTS + 1)), ("pad", C.c_int32),
                ("seg_script", (C.c_int32 * NAV_MAX_SEGMENTS) * NAV_MAX_NAVIGATORS),
                ("grid", C.c_void_p), ("free", C.c_void_p), ("snap", C.c_void_p), ("hops", C.c_void_p), ("slot_map", C.c_void_p),
                ("team_positions", C.c_void_p), ("uniform", C.c_void_p), ("actions", C.c_void_p), ("nav_hops", C.c_void_p)]


def nav_build(grid_host, grid, free, hops) -> None:
    """The all-pairs hop table of a batch of map grids in one launch (``cat_render_nav_build``): ``grid_host`` int32 [M, 4] NumPy (Wc, Hc,
    cell_off, hops_off), ``grid`` the same on the device, ``free`` uint8 [sum C], ``hops`` uint16 / int16 [sum C^2] (written)."""
    import numpy as np
    import torch
    M = grid_host.shape[0]
    assert grid_host.dtype == np.int32 and grid_host.shape == (M, 4) and grid_host.flags.c_contiguous
    assert grid.dtype == torch.int32 and tuple(grid.shape) == (M, 4) and grid.is_contiguous()
    cells = int((grid_host[:, 0].astype(np.int64) * grid_host[:, 1]).sum())
    entries = int(((grid_host[:, 0].astype(np.int64) * grid_host[:, 1]) ** 2).sum())
    assert free.dtype == torch.uint8 and free.numel() == cells and free.is_contiguous()
    assert hops.element_size() == 2 and hops.numel() == entries and hops.is_contiguous()
    assert grid.device == free.device == hops.device
    a = NavBuildArgs(M, 0, grid_host.ctypes.data, grid.data_ptr(), free.data_ptr(), hops.data_ptr())
    _check(lib().cat_render_nav_build(C.byref(a), _stream()), "cat_render_nav_build")


class NavTable:
    """A checked segment table of ``cat_render_nav_step_args`` in the C struct's own arrays (``nav_table`` makes it)."""

    def __init__(self, S: int, start, rows):
        self.S, self.start, self.rows = S, start, rows
        self.seg_start = (C.c_int32 * (NAV_MAX_SEGMENTS + 1))(*start)
        self.seg_script = ((C.c_int32 * NAV_MAX_SEGMENTS) * NAV_MAX_NAVIGATORS)(*[(C.c_int32 * NAV_MAX_SEGMENTS)(*row) for row in rows])


def nav_table(N: int, G: int, bounds, rows) -> NavTable:
    """The segment table of ``cat_render_nav_step_args`` checked by the C entry's rules: ``bounds`` S + 1 row bounds (``_check_bounds``),
    ``rows`` [G][S] scripts in {-1, NAV_PURSUE, NAV_FLEE}.  Raises ValueError."""
    start = [int(v) for v in bounds]
    _check_bounds(N, start, NAV_MAX_SEGMENTS)
    S = len(start) - 1
    table = [[int(v) for v in row] for row in rows]
    if not 1 <= G <= NAV_MAX_NAVIGATORS or len(table) != G or any(len(row) != S for row in table):
        raise ValueError(f"the scripts must be [{G}][{S}] with 1 <= G <= {NAV_MAX_NAVIGATORS}")
    if any(v not in (-1, NAV_PURSUE, NAV_FLEE) for row in table for v in row):
        raise ValueError("a script outside {-1, 0, 1}")
    return NavTable(S, start, table)


def nav_step(team_positions, uniform, field, agent_indices, opp_masks, table, actions, nav_hops=None) -> None:
    """One tick of the navigators in one launch (``cat_render_nav_step``): team_positions f16 [N, A, 2], uniform fp32 [G, N], ``field`` with
    the device tensors grid / free / snap / hops / slot_map of ``navigation.NavField`` and its ``cell``, ``table`` a ``NavTable`` for these N
    and G; actions int32 [N, A]: column ``agent_indices[g]`` receives navigator g's action where its script is not -1; nav_hops int32
    [G, N] or None."""
    import torch
    N, A, _ = team_positions.shape
    G = len(agent_indices)
    assert team_positions.dtype == torch.float16 and team_positions.shape == (N, A, 2) and team_positions.is_contiguous()
    assert isinstance(table, NavTable) and table.start[-1] == N and len(table.rows) == G == len(opp_masks)
    assert uniform.dtype == torch.float32 and uniform.shape == (G, N) and uniform.is_contiguous()
    assert actions.dtype == torch.int32 and actions.shape == (N, A) and actions.is_contiguous()
    assert nav_hops is None or (nav_hops.dtype == torch.int32 and nav_hops.shape == (G, N) and nav_hops.is_contiguous())
    assert field.slot_map.dtype == torch.int32 and field.slot_map.shape == (N,) and field.slot_map.is_contiguous()
    assert all(t.device == actions.device for t in (team_positions, uniform, field.grid, field.free, field.snap, field.hops, field.slot_map))
    pad = [0] * (NAV_MAX_NAVIGATORS - G)
    a = NavStepArgs(N, A, G, table.S, field.grid.shape[0], int(field.cell), (C.c_int32 * NAV_MAX_NAVIGATORS)(*agent_indices, *pad),
                    (C.c_uint32 * NAV_MAX_NAVIGATORS)(*opp_masks, *pad), table.seg_start, 0, table.seg_script,
                    field.grid.data_ptr(), field.free.data_ptr(), field.snap.data_ptr(), field.hops.data_ptr(), field.slot_map.data_ptr(),
                    team_positions.data_ptr(), uniform.data_ptr(), actions.data_ptr(), _ptr(nav_hops))
    _check(lib().cat_render_nav_step(C.byref(a), _stream()), "cat_render_nav_step")


class NavShapeArgs(C.Structure):
    """include/cat_render.h cat_render_nav_shape_args."""
    _fields_ = [("N", C.c_int32), ("A", C.c_int32), ("G", C.c_int32), ("n_maps", C.c_int32), ("cell", C.c_int32), ("cap", C.c_int32),
                ("prime", C.c_int32), ("pad", C.c_int32),
                ("agent", C.c_int32 * NAV_MAX_NAVIGATORS), ("opp_mask", C.c_uint32 * NAV_MAX_NAVIGATORS), ("coef", C.c_float * NAV_MAX_NAVIGATORS),
                ("gamma", C.c_float), ("pad2", C.c_int32),
                ("grid", C.c_void_p), ("snap", C.c_void_p), ("hops", C.c_void_p), ("slot_map", C.c_void_p),
                ("team_positions", C.c_void_p), ("final_positions", C.c_void_p), ("terminated", C.c_void_p), ("truncated", C.c_void_p),
                ("reward_out", C.c_void_p), ("sr_g", C.c_int64), ("shaping_out", C.c_void_p), ("ss_g", C.c_int64), ("hops_prev", C.c_void_p)]


def _rows_gn(t, G: int, N: int, name: str):
    """(pointer, row stride in elements) of an fp32 [G, N] tensor whose rows are contiguous (any row stride: a [G, T, N] buffer's [:, t])."""
    import torch
    assert t.dtype == torch.float32 and tuple(t.shape) == (G, N) and (N == 1 or t.stride(1) == 1), f"{name}: fp32 [G, N] with contiguous rows"
    return t.data_ptr(), int(t.stride(0))


def nav_shape(team_positions, field, agent_indices, opp_masks, coef, gamma: float, cap: int, hops_prev, *, final_positions=None,
              terminated=None, truncated=None, reward_out=None, shaping_out=None, prime: bool = False) -> None:
    """One tick of geodesic reward shaping in one launch (``cat_render_nav_shape``; ``navigation.shaping_step`` is its definition):
    team_positions / final_positions f16 [N, A, 2], terminated / truncated u8 [N], ``field`` as in ``nav_step``, per shaped agent its column,
    opponent bitmask and fp32 coefficient; hops_prev int32 [G, N] (read and rewritten), reward_out fp32 [G, N] with contiguous rows at any
    row stride (takes ``+ F``), shaping_out the same or None (takes ``F``).  ``prime``: only hops_prev is written and the other buffers may
    be None."""
    import torch
    N, A, _ = team_positions.shape
    G = len(agent_indices)
    assert 1 <= G <= NAV_MAX_NAVIGATORS and len(opp_masks) == G == len(coef)
    assert team_positions.dtype == torch.float16 and team_positions.shape == (N, A, 2) and team_positions.is_contiguous()
    assert hops_prev.dtype == torch.int32 and hops_prev.shape == (G, N) and hops_prev.is_contiguous()
    assert field.slot_map.dtype == torch.int32 and field.slot_map.shape == (N,) and field.slot_map.is_contiguous()
    tensors = [team_positions, hops_prev, field.grid, field.snap, field.hops, field.slot_map]
    rp = sp = sr = ss = 0
    if not prime:
        assert final_positions is not None and final_positions.dtype == torch.float16 and final_positions.shape == (N, A, 2) and final_positions.is_contiguous()
        for f in (terminated, truncated):
            assert f is not None and f.dtype == torch.uint8 and f.shape == (N,) and f.is_contiguous()
        rp, sr = _rows_gn(reward_out, G, N, "reward_out")
        tensors += [final_positions, terminated, truncated, reward_out]
        if shaping_out is not None:
            sp, ss = _rows_gn(shaping_out, G, N, "shaping_out")
            tensors.append(shaping_out)
    assert all(t.device == team_positions.device for t in tensors)
    pad = [0] * (NAV_MAX_NAVIGATORS - G)
    a = NavShapeArgs(N, A, G, field.grid.shape[0], int(field.cell), int(cap), int(bool(prime)), 0,
                     (C.c_int32 * NAV_MAX_NAVIGATORS)(*agent_indices, *pad), (C.c_uint32 * NAV_MAX_NAVIGATORS)(*opp_masks, *pad),
                     (C.c_float * NAV_MAX_NAVIGATORS)(*[float(c) for c in coef], *pad), float(gamma), 0,
                     field.grid.data_ptr(), field.snap.data_ptr(), field.hops.data_ptr(), field.slot_map.data_ptr(),
                     team_positions.data_ptr(), _ptr(None if prime else final_positions), _ptr(None if prime else terminated),
                     _ptr(None if prime else truncated), rp or None, sr, sp or None, ss, hops_prev.data_ptr())
    _check(lib().cat_render_nav_shape(C.byref(a), _stream()), "cat_render_nav_shape")


class NavSpawnArgs(C.Structure):
    """include/cat_render.h cat_render_nav_spawn_args."""
    _fields_ = [("N", C.c_int32), ("A", C.c_int32), ("n_cops", C.c_int32), ("n_maps", C.c_int32), ("cell", C.c_int32), ("pad", C.c_int32),
                ("grid", C.c_void_p), ("free", C.c_void_p), ("hops", C.c_void_p), ("slot_map", C.c_void_p),
                ("mask", C.c_void_p), ("band", C.c_void_p), ("uniform", C.c_void_p), ("positions", C.c_void_p), ("placed", C.c_void_p)]


def nav_spawn(mask, uniform, band, field, n_cops: int, positions, placed) -> None:
    """Start states of the geodesic curriculum in one launch (``cat_render_nav_spawn``; ``navigation.spawn_step`` is its definition): mask u8
    [N], uniform fp32 [A, N], band int32 [N, 2], ``field`` as in ``nav_step``; positions f64 [N, A, 2] (rows with ``placed[n] == 1`` are
    written, no other) and placed u8 [N] (every row)."""
    import torch
    A, N = uniform.shape
    assert mask.dtype == torch.uint8 and mask.shape == (N,) and mask.is_contiguous()
    assert uniform.dtype == torch.float32 and uniform.is_contiguous()
    assert band.dtype == torch.int32 and band.shape == (N, 2) and band.is_contiguous()
    assert positions.dtype == torch.float64 and positions.shape == (N, A, 2) and positions.is_contiguous()
    assert placed.dtype == torch.uint8 and placed.shape == (N,) and placed.is_contiguous()
    assert field.slot_map.dtype == torch.int32 and field.slot_map.shape == (N,) and field.slot_map.is_contiguous()
    assert all(t.device == positions.device for t in (mask, uniform, band, placed, field.grid, field.free, field.hops, field.slot_map))
    a = NavSpawnArgs(N, A, int(n_cops), field.grid.shape[0], int(field.cell), 0, field.grid.data_ptr(), field.free.data_ptr(),
                     field.hops.data_ptr(), field.slot_map.data_ptr(), mask.data_ptr(), band.data_ptr(), uniform.data_ptr(),
                     positions.data_ptr(), placed.data_ptr())
    _check(lib().cat_render_nav_spawn(C.byref(a), _stream()), "cat_render_nav_spawn")


# ---------------------------------------------------------------------------------------------- scripted opponents
SCRIPT_CHASE, SCRIPT_EVADE = 0, 1   # CAT_ROLLOUT_CHASE / CAT_ROLLOUT_EVADE; -1: not scripted in that segment
SCRIPTED_MAX_SEGMENTS = 32          # CAT_ROLLOUT_MAX_SEGMENTS (= ACT_MAX_SEGMENTS)
SCRIPTED_MIN_RAYS, SCRIPTED_MAX_RAYS = 8, 1024


class ScriptedArgs(C.Structure):
    """include/cat_rollout.h cat_rollout_scripted_args."""
    _fields_ = [("N", C.c_int32), ("A", C.c_int32), ("R", C.c_int32), ("G", C.c_int32), ("agent", C.c_int32 * 8), ("target", C.c_int32 * 8),
                ("memory_ticks", C.c_int32), ("clear_min", C.c_float), ("turn_prob", C.c_float), ("S", C.c_int32),
                ("seg_start", C.c_int32 * (SCRIPTED_MAX_SEGMENTS + 1)), ("seg_script", (C.c_int32 * SCRIPTED_MAX_SEGMENTS) * 8),
                ("obs_distance", C.c_void_p), ("obs_type", C.c_void_p), ("uniform", C.c_void_p), ("keep", C.c_void_p),
                ("state", C.c_void_p), ("actions", C.c_void_p)]


class ScriptedTable:
    """A checked segment table of ``cat_rollout_scripted_args`` in the C struct's own arrays (``scripted_table`` makes it)."""

    def __init__(self, S: int, start, rows):
        self.S, self.start, self.rows = S, start, rows
        self.seg_start = (C.c_int32 * (SCRIPTED_MAX_SEGMENTS + 1))(*start)
        self.seg_script = ((C.c_int32 * SCRIPTED_MAX_SEGMENTS) * 8)(*[(C.c_int32 * SCRIPTED_MAX_SEGMENTS)(*row) for row in rows])


def scripted_table(N: int, G: int, bounds, rows) -> ScriptedTable:
    """The segment table of ``cat_rollout_scripted_args`` checked by the C entry's rules: ``bounds`` S + 1 row bounds (``_check_bounds``),
    ``rows`` [G][S] scripts in {-1, SCRIPT_CHASE, SCRIPT_EVADE}.  Raises ValueError."""
    start = [int(v) for v in bounds]
    _check_bounds(N, start, SCRIPTED_MAX_SEGMENTS)
    S = len(start) - 1
    table = [[int(v) for v in row] for row in rows]
    if not 1 <= G <= 8 or len(table) != G or any(len(row) != S for row in table):
        raise ValueError(f"the scripts must be [{G}][{S}] with 1 <= G <= 8")
    if any(v not in (-1, SCRIPT_CHASE, SCRIPT_EVADE) for row in table for v in row):
        raise ValueError("a script outside {-1, 0, 1}")
    return ScriptedTable(S, start, table)


def rollout_scripted(raw, agent_indices, targets, table, uniform, keep, state, actions, memory_ticks: int = 30, clear_min: float = 12.0,
                     turn_prob: float = 0.02) -> None:
    """One tick of the scripted opponents in one launch (include/cat_rollout.h, ``cat_rollout_scripted``).  raw = the env core's output
    buffers (obs_distance f16 / obs_type u8 [N, A, R]); ``targets[g]``: the type code policy g looks for; ``table``: a ``ScriptedTable``
    for these N and G; uniform fp32 [G, N]; keep fp32 [N] or None; state int32 [G, N, 4] updated in place; actions int32 [N, A]: column
    ``agent_indices[g]`` receives policy g's action where its script is not -1."""
    import torch
    od, ot = raw["obs_distance"], raw["obs_type"]
    N, A, R = od.shape
    G = len(agent_indices)
    assert od.dtype == torch.float16 and ot.dtype == torch.uint8 and od.is_contiguous() and ot.is_contiguous() and ot.shape == od.shape
    assert isinstance(table, ScriptedTable) and table.start[-1] == N and len(table.rows) == G == len(targets)
    assert uniform.dtype == torch.float32 and uniform.shape == (G, N) and uniform.is_contiguous()
    assert keep is None or (keep.dtype == torch.float32 and keep.numel() == N and keep.is_contiguous())
    assert state.dtype == torch.int32 and state.shape == (G, N, 4) and state.is_contiguous()
    assert actions.dtype == torch.int32 and actions.shape == (N, A) and actions.is_contiguous()
    a = ScriptedArgs(N, A, R, G, (C.c_int32 * 8)(*agent_indices), (C.c_int32 * 8)(*targets), int(memory_ticks), float(clear_min), float(turn_prob),
                     table.S, table.seg_start, table.seg_script, od.data_ptr(), ot.data_ptr(), uniform.data_ptr(), _ptr(keep), state.data_ptr(),
                     actions.data_ptr())
    _check(lib().cat_rollout_scripted(C.byref(a), _stream()), "cat_rollout_scripted")


# ---------------------------------------------------------------------------------------------- the fused act tick
ACT_PARAM_FIELDS = ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "fc_w", "fc_b", "w_ih", "w_hh", "b_ih", "b_hh",
                    "head0_w", "head0_b", "head1_w", "head1_b", "head2_w", "head2_b")
# models.LSTMPolicy's parameter names in the order of ACT_PARAM_FIELDS
ACT_PARAM_NAMES = ("features_extractor.0.weight", "features_extractor.0.bias", "features_extractor.2.weight", "features_extractor.2.bias",
                   "features_extractor.5.weight", "features_extractor.5.bias", "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0",
                   "lstm.bias_hh_l0", "policy_head.0.weight", "policy_head.0.bias", "policy_head.2.weight", "policy_head.2.bias",
                   "policy_head.4.weight", "policy_head.4.bias")


class ActDims(C.Structure):
    _fields_ = [("G", C.c_int32), ("N", C.c_int32), ("A", C.c_int32), ("R", C.c_int32)]


class ActParams(C.Structure):
    """include/cat_act.h cat_act_params."""
    _fields_ = [(n, C.c_void_p) for n in ACT_PARAM_FIELDS] + [("stride", C.c_int64)]


class ActArgs(C.Structure):
    """include/cat_act.h cat_act_args."""
    _fields_ = [("d", ActDims), ("agent", C.c_int32 * ACT_MAX_AGENTS), ("mode", C.c_int32), ("random_mask", C.c_uint32), ("row_tile", C.c_int32),
                ("distance_scale", C.c_float), ("type_scale", C.c_float), ("pad", C.c_int32),
                ("obs_distance", C.c_void_p), ("obs_type", C.c_void_p), ("p", ActParams), ("h", C.c_void_p), ("c", C.c_void_p),
                ("keep", C.c_void_p), ("uniform", C.c_void_p), ("actions", C.c_void_p), ("logits_out", C.c_void_p), ("logp_out", C.c_void_p)]


class ActCollectArgs(C.Structure):
    """include/cat_act.h cat_act_collect_args."""
    _fields_ = [("base", ActArgs), ("n_cops", C.c_int32), ("first_agent_state", C.c_int32), ("shared_distance", C.c_void_p), ("shared_type", C.c_void_p),
                ("policy_in", C.c_void_p), ("sp_g", C.c_int64), ("sp_n", C.c_int64), ("value_in", C.c_void_p), ("sv_g", C.c_int64), ("sv_n", C.c_int64),
                ("act_out", C.c_void_p), ("sa_g", C.c_int64), ("logp_out", C.c_void_p), ("sl_g", C.c_int64), ("h0_out", C.c_void_p), ("c0_out", C.c_void_p)]


class ActLeagueArgs(C.Structure):
    """include/cat_act.h cat_act_league_args."""
    _fields_ = [("base", ActArgs), ("S", C.c_int32), ("sets", C.c_int32), ("seg_start", C.c_int32 * (ACT_MAX_SEGMENTS + 1)),
                ("seg_set", (C.c_int32 * ACT_MAX_SEGMENTS) * ACT_MAX_AGENTS)]


def act_supported(G: int, N: int, A: int, R: int) -> bool:
    d = ActDims(G, N, A, R)
    return bool(lib().cat_act_supported(C.byref(d)))


def act_params(params) -> ActParams:
    """``params``: models.LSTMPolicy's parameter name -> stacked bf16 view [G, ...] (``FlatParams.views`` without the ``policy.`` prefix)
    whose per-network blocks are contiguous and share ONE stride between the networks (rows of one flat buffer)."""
    import torch
    ts = [params[n] for n in ACT_PARAM_NAMES]
    stride = ts[0].stride(0)
    for t in ts:
        assert t.dtype == torch.bfloat16 and t[0].is_contiguous() and (t.shape[0] == 1 or t.stride(0) == stride) and t.data_ptr() % 16 == 0
    return ActParams(*[t.data_ptr() for t in ts], stride)


def act_step(raw, agent_indices, params, h, c, keep, uniform, actions, distance_scale: float = 1.0, type_scale: float = 1.0, greedy: bool = False,
             random_mask: int = 0, logits_out=None, logp_out=None, row_tile: int = 0) -> None:
    """One act tick of the G stacked recurrent policies in one launch (include/cat_act.h).  raw = the env core's output buffers
    (``VecCopsEnv.raw_outputs()``: obs_distance f16 / obs_type u8 [N, A, R]); params = ``act_params(...)`` (or the mapping it takes); h, c bf16
    [G, N, 128] updated in place; keep fp32 [N] or None; uniform fp32 [G, N]; actions int32 [N, A]: column ``agent_indices[g]`` receives
    policy g's action; logits_out bf16 [G, N, 4] / logp_out fp32 [G, N] optional."""
    _check(lib().cat_act_step(C.byref(_act_args(raw, agent_indices, params, h, c, keep, uniform, actions, distance_scale, type_scale, greedy, random_mask,
                                                logits_out, logp_out, row_tile)), _stream()), "cat_act_step")


def _act_args(raw, agent_indices, params, h, c, keep, uniform, actions, distance_scale, type_scale, greedy, random_mask, logits_out, logp_out,
              row_tile) -> ActArgs:
    """The checked ``cat_act_args`` of ``act_step`` / ``act_league_step``."""
    import torch
    od, ot = raw["obs_distance"], raw["obs_type"]
    N, A, R = od.shape
    G = len(agent_indices)
    assert od.dtype == torch.float16 and ot.dtype == torch.uint8 and od.is_contiguous() and ot.is_contiguous() and ot.shape == od.shape
    assert 1 <= G <= ACT_MAX_AGENTS and act_supported(G, N, A, R), f"cat_act_step does not take G={G}, A={A}, R={R}"
    for t in (h, c):
        assert t.dtype == torch.bfloat16 and t.shape == (G, N, HIDDEN) and t.is_contiguous()
    assert keep is None or (keep.dtype == torch.float32 and keep.numel() == N and keep.is_contiguous())
    assert uniform.dtype == torch.float32 and uniform.shape == (G, N) and uniform.is_contiguous()
    assert actions.dtype == torch.int32 and actions.shape == (N, A) and actions.is_contiguous()
    assert logits_out is None or (logits_out.dtype == torch.bfloat16 and logits_out.shape == (G, N, 4) and logits_out.is_contiguous())
    assert logp_out is None or (logp_out.dtype == torch.float32 and logp_out.shape == (G, N) and logp_out.is_contiguous())
    p = params if isinstance(params, ActParams) else act_params(params)
    return ActArgs(ActDims(G, N, A, R), (C.c_int32 * ACT_MAX_AGENTS)(*agent_indices), ACT_GREEDY if greedy else ACT_SAMPLE, int(random_mask), int(row_tile),
                   distance_scale, type_scale, 0, od.data_ptr(), ot.data_ptr(), p, h.data_ptr(), c.data_ptr(), _ptr(keep), uniform.data_ptr(),
                   actions.data_ptr(), _ptr(logits_out), _ptr(logp_out))


def act_collect_step(raw, agent_indices, params, h, c, keep, uniform, actions, n_cops: int, first_agent_state: bool, policy_in, value_in, act_out,
                     logp_out, h0_out=None, c0_out=None, distance_scale: float = 1.0, type_scale: float = 1.0, logits_out=None, base_logp_out=None,
                     row_tile: int = 0) -> None:
    """``act_step`` (sampled, no random agents) that also writes what a rollout keeps of the tick, in one launch (include/cat_act.h,
    ``cat_act_collect_step``).  raw additionally holds shared_distance f16 / shared_type u8 [N, 2, R]; policy_in bf16 [G, N, 2R] and value_in bf16
    [G, N, 4R]: views with contiguous rows whose outer strides are multiples of 4 elements (``rollout_pack``'s rows); act_out int64 / logp_out fp32
    [G, N] row-strided views (``rollout_sample``'s); h0_out, c0_out bf16 [G, N, 128] contiguous, both or neither: h and c as they stood before the
    tick.  ``logits_out`` / ``base_logp_out``: ``act_step``'s optional contiguous outputs."""
    import torch
    sd, st = raw["shared_distance"], raw["shared_type"]
    a = ActCollectArgs()
    a.base = _act_args(raw, agent_indices, params, h, c, keep, uniform, actions, distance_scale, type_scale, False, 0, logits_out, base_logp_out, row_tile)
    G, N, R = a.base.d.G, a.base.d.N, a.base.d.R
    assert sd.dtype == torch.float16 and st.dtype == torch.uint8 and sd.shape == st.shape == (N, 2, R) and sd.is_contiguous() and st.is_contiguous()
    for t, w in ((policy_in, 2 * R), (value_in, 4 * R)):
        assert t.dtype == torch.bfloat16 and t.shape == (G, N, w) and t.stride(2) == 1
    assert act_out.dtype == torch.int64 and act_out.shape == (G, N) and act_out.stride(1) == 1
    assert logp_out.dtype == torch.float32 and logp_out.shape == (G, N) and logp_out.stride(1) == 1
    for t in (h0_out, c0_out):
        assert t is None or (t.dtype == torch.bfloat16 and t.shape == (G, N, HIDDEN) and t.is_contiguous())
    a.n_cops, a.first_agent_state, a.shared_distance, a.shared_type = int(n_cops), 1 if first_agent_state else 0, sd.data_ptr(), st.data_ptr()
    a.policy_in, a.sp_g, a.sp_n = policy_in.data_ptr(), policy_in.stride(0), policy_in.stride(1)
    a.value_in, a.sv_g, a.sv_n = value_in.data_ptr(), value_in.stride(0), value_in.stride(1)
    a.act_out, a.sa_g, a.logp_out, a.sl_g = act_out.data_ptr(), act_out.stride(0), logp_out.data_ptr(), logp_out.stride(0)
    a.h0_out, a.c0_out = _ptr(h0_out) or None, _ptr(c0_out) or None
    _check(lib().cat_act_collect_step(C.byref(a), _stream()), "cat_act_collect_step")


class LeagueTable:
    """A checked segment table in the C struct's own arrays (``league_table`` makes it; ``act_league_step`` copies it in whole)."""

    def __init__(self, S: int, sets: int, start, table):
        self.S, self.sets, self.start, self.table = S, sets, start, table
        self.seg_start = (C.c_int32 * (ACT_MAX_SEGMENTS + 1))(*start)
        self.seg_set = ((C.c_int32 * ACT_MAX_SEGMENTS) * ACT_MAX_AGENTS)(*[(C.c_int32 * ACT_MAX_SEGMENTS)(*row) for row in table])


def league_table(N: int, G: int, sets: int, seg_start, seg_set) -> LeagueTable:
    """The segment table of ``cat_act_league_args`` checked by the C entry's rules: ``seg_start`` S + 1 row bounds (0 first, N last, strictly
    increasing, 1 <= S <= ACT_MAX_SEGMENTS), ``seg_set`` [G][S] set indices in [-1, sets) (-1: uniformly random).  Raises ValueError."""
    start = [int(v) for v in seg_start]
    _check_bounds(N, start, ACT_MAX_SEGMENTS)
    S = len(start) - 1
    if sets < 1:
        raise ValueError("the bank needs at least one parameter set")
    table = [[int(v) for v in row] for row in seg_set]
    if len(table) != G or any(len(row) != S for row in table):
        raise ValueError(f"seg_set must be [{G}][{S}]")
    if any(not -1 <= v < sets for row in table for v in row):
        raise ValueError(f"a set index outside [-1, {sets})")
    return LeagueTable(S, int(sets), start, table)


def act_league_step(raw, agent_indices, bank_params, sets: int, seg_start, seg_set, h, c, keep, uniform, actions, distance_scale: float = 1.0,
                    type_scale: float = 1.0, greedy: bool = False, logits_out=None, logp_out=None, row_tile: int = 0) -> None:
    """``act_step`` with per-segment parameter sets in one launch (include/cat_act.h, ``cat_act_league_step``).  bank_params =
    ``act_params(...)`` over the bank's ``[sets, ...]`` views: set k of every block at pointer + k * stride.  Rows ``seg_start[s] ..
    seg_start[s + 1] - 1`` of policy g are played by set ``seg_set[g][s]``, or uniformly at random where that is -1 (state and optional
    outputs of those rows untouched).  ``seg_start`` may be a ``LeagueTable`` made for these N, G and sets (``seg_set`` is then ignored).
    Everything else as in ``act_step``; there is no ``random_mask``."""
    G, N = uniform.shape
    t = seg_start if isinstance(seg_start, LeagueTable) else league_table(N, len(agent_indices), sets, seg_start, seg_set)
    assert G == len(agent_indices) and t.start[-1] == N and len(t.table) == G and t.sets == sets
    a = ActLeagueArgs()
    a.base = _act_args(raw, agent_indices, bank_params, h, c, keep, uniform, actions, distance_scale, type_scale, greedy, 0, logits_out, logp_out, row_tile)
    a.S, a.sets, a.seg_start, a.seg_set = t.S, t.sets, t.seg_start, t.seg_set
    _check(lib().cat_act_league_step(C.byref(a), _stream()), "cat_act_league_step")
