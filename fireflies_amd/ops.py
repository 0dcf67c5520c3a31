"""Tensor-level wrappers over the C ABI (include/ffx.h) — plumbing only.

PyTorch is used for device memory and the current HIP stream; every arithmetic step happens in
libffx_hip.so.  All functions require contiguous tensors on a HIP device and raise otherwise.
"""
import ctypes as C
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _abi
from ._lib import api

REDUCE = {"sum": _abi.REDUCE_SUM, "softor": _abi.REDUCE_SOFTOR}


def _dev_index(device=None):
    if device is None:
        return torch.cuda.current_device()
    if isinstance(device, int):
        return device
    idx = torch.device(device).index
    return torch.cuda.current_device() if idx is None else idx


def _stream(device=None):
    """the caller's current HIP stream on `device` (default: the current device) as a raw handle.
    (torch.cuda.current_stream() builds a Stream object through several Python layers: 10 us per call,
    seven calls per render step; the raw query is one C call.)"""
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(_dev_index(device)))


_STREAM_OBJECTS = {}


def _stream_obj(device=None):
    """torch Stream object of the caller's current stream (for event record / wait), cached by raw handle"""
    idx = _dev_index(device)
    raw = torch._C._cuda_getCurrentRawStream(idx)
    s = _STREAM_OBJECTS.get((idx, raw))
    if s is None:
        s = torch.cuda.current_stream(idx)
        if len(_STREAM_OBJECTS) > 64:
            _STREAM_OBJECTS.clear()
        _STREAM_OBJECTS[(idx, raw)] = s
    return s


def _dev(t, dtype=torch.float32, name="tensor"):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: must live on a HIP device (got {t.device}); fireflies_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return C.c_void_p(t.data_ptr())


def _m16(m):
    if isinstance(m, torch.Tensor):
        m = m.detach().cpu().numpy()
    a = np.asarray(m, dtype=np.float32).reshape(-1)
    if a.size != 16:
        raise ValueError("expected a 4x4 matrix")
    return (C.c_float * 16)(*a.tolist())


def _reduce(reduce):
    if isinstance(reduce, str):
        return REDUCE[reduce]
    return int(reduce)


# ------------------------------------------------------------------ K1
def project_rays_fwd(rays, KF):
    out = torch.empty_like(rays)
    api().call("ffx_project_rays_fwd", _dev(rays, name="rays"), rays.shape[0], _m16(KF), _dev(out), _stream())
    return out


def project_rays_bwd(rays, KF, gpts):
    out = torch.empty_like(rays)
    api().call("ffx_project_rays_bwd", _dev(rays, name="rays"), rays.shape[0], _m16(KF), _dev(gpts, name="gpts"), _dev(out), _stream())
    return out


def transform_points(pts, M, mode=0):
    out = torch.empty_like(pts)
    api().call("ffx_transform_points", _dev(pts, name="pts"), pts.shape[0], _m16(M), mode, _dev(out), _stream())
    return out


def l1_value_grad(a, b, weight=1.0, acc=None):
    """weight * L1Loss(a, b) (a 0-dim view into the workspace) and its gradient with respect to `a`; acc (a float32 tensor): the value is
    also added to acc[0] by the same launches"""
    ws = torch.empty(257, dtype=torch.float32, device=a.device)
    g = torch.empty_like(a)
    if acc is not None:
        api().call("ffx_l1_value_grad_acc", _dev(a, name="a"), _dev(b, name="b"), a.numel(), float(weight), _dev(ws), _dev(g), _dev(acc.reshape(-1), name="acc"), _stream())
    else:
        api().call("ffx_l1_value_grad", _dev(a, name="a"), _dev(b, name="b"), a.numel(), float(weight), _dev(ws), _dev(g), _stream())
    return ws[0], g


def clamp_to_fov_(rays, KF, KF_inv, lo, hi, n_normalize=1):
    """in place: Laser.clamp_to_fov (+ n_normalize - 1 further normalisations) in one launch"""
    api().call("ffx_clamp_to_fov", _dev(rays, name="rays"), rays.shape[0], _m16(KF), _m16(KF_inv), float(lo), float(hi), int(n_normalize), _stream())
    return rays


# ------------------------------------------------------------------ fused pattern side of an optimisation step
def pattern_ws_floats(size0, size1):
    return int(api().lib.ffx_pattern_ws_floats(int(size0), int(size1)))


def pattern_fwd(rays, KF, sigma, size0, size1, want_softor=True, out=None, zero=None):
    """K1 + K2(sum) + K2(softor) + partial sums of L1(softor, sum) in one launch -> (pts [n,2], tsum, tsor, ws).
    `out`: optional tuple of tensors to reuse.  `zero`: a float32 tensor the same launch clears."""
    n = rays.shape[0]
    if out is None:
        pts = torch.empty((n, 2), dtype=torch.float32, device=rays.device)
        tsum = torch.empty((size1, size0), dtype=torch.float32, device=rays.device)
        tsor = torch.empty((size1, size0), dtype=torch.float32, device=rays.device) if want_softor else None
        ws = torch.empty(pattern_ws_floats(size0, size1), dtype=torch.float32, device=rays.device) if want_softor else None
    else:
        pts, tsum, tsor, ws = out
    api().call("ffx_pattern_fwd", _dev(rays, name="rays"), n, _m16(KF), float(sigma), int(size0), int(size1), int(bool(want_softor)), _dev(pts), _dev(tsum),
               _dev(tsor) if want_softor else None, _dev(ws) if want_softor else None, _dev(zero, name="zero") if zero is not None else None,
               int(zero.numel()) if zero is not None else 0, _stream())
    return pts, tsum, tsor, ws


def pattern_bwd(rays, KF, sigma, size0, size1, tsum, tsor, gts, reg_weight, ws, loss_in=None, loss_div=1.0):
    """K2-bwd of the data term (gts on the sum texture) and of reg_weight * L1(softor, sum), each through K1-bwd, in
    one launch -> (grays_data or None, grays_reg or None, [3] tensor: regulariser value, and — if `loss_in`, a tensor of
    partial sums of the data term (or one value), is given — sum(loss_in) / loss_div + regulariser, and sum(loss_in))"""
    n = rays.shape[0]
    gd = torch.empty((n, 3), dtype=torch.float32, device=rays.device) if gts is not None else None
    gr = torch.empty((n, 3), dtype=torch.float32, device=rays.device) if reg_weight > 0 else None
    val = torch.empty(3, dtype=torch.float32, device=rays.device)
    api().call("ffx_pattern_bwd", _dev(rays, name="rays"), n, _m16(KF), float(sigma), int(size0), int(size1), _dev(tsum, name="tsum"),
               _dev(tsor, name="tsor") if tsor is not None else None, _dev(gts, name="gts") if gts is not None else None, float(reg_weight),
               _dev(ws, name="ws") if ws is not None else None, _dev(gd) if gd is not None else None, _dev(gr) if gr is not None else None, _dev(val),
               _dev(loss_in, name="loss_in") if loss_in is not None else None, int(loss_in.numel()) if loss_in is not None else 0, float(loss_div), _stream())
    return gd, gr, val


def pattern_fwd_blur(rays, KF, sigma, size0, size1, ksize, blur_sigma, want_softor=True, out=None, zero=None):
    """pattern_fwd + tex = blur_fwd(tsum, ksize, blur_sigma) in one launch (ffx_pattern_fwd_blur) -> (pts, tsum, tsor, ws, tex); `out`: the five
    tensors to reuse."""
    n = rays.shape[0]
    if out is None:
        pts = torch.empty((n, 2), dtype=torch.float32, device=rays.device)
        tsum = torch.empty((size1, size0), dtype=torch.float32, device=rays.device)
        tsor = torch.empty((size1, size0), dtype=torch.float32, device=rays.device) if want_softor else None
        ws = torch.empty(pattern_ws_floats(size0, size1), dtype=torch.float32, device=rays.device) if want_softor else None
        tex = torch.empty((size1, size0), dtype=torch.float32, device=rays.device)
    else:
        pts, tsum, tsor, ws, tex = out
    api().call("ffx_pattern_fwd_blur", _dev(rays, name="rays"), n, _m16(KF), float(sigma), int(size0), int(size1), int(bool(want_softor)), _dev(pts), _dev(tsum),
               _dev(tsor) if want_softor else None, _dev(ws) if want_softor else None, _dev(zero, name="zero") if zero is not None else None,
               int(zero.numel()) if zero is not None else 0, int(ksize), float(blur_sigma), _dev(tex), _stream())
    return pts, tsum, tsor, ws, tex


def pattern_bwd_blur(rays, KF, sigma, size0, size1, tsum, tsor, gtex, reg_weight, ws, ksize, blur_sigma, loss_in=None, loss_div=1.0, adam=None, scratch=None):
    """pattern_bwd with K3^T in front (gtex: the gradient on the BLURRED texture; ksize 0: on tsum) and, with `adam` (an _abi.AdamArgs whose
    rays field names `rays`), the Adam + clamp_to_fov update behind it — one launch (ffx_pattern_bwd_blur).  -> (grays_data, grays_reg, [3])"""
    n = rays.shape[0]
    gd = torch.empty((n, 3), dtype=torch.float32, device=rays.device) if gtex is not None else None
    gr = torch.empty((n, 3), dtype=torch.float32, device=rays.device) if reg_weight > 0 else None
    val = torch.empty(3, dtype=torch.float32, device=rays.device)
    api().call("ffx_pattern_bwd_blur", _dev(rays, name="rays"), n, _m16(KF), float(sigma), int(size0), int(size1), _dev(tsum, name="tsum"),
               _dev(tsor, name="tsor") if tsor is not None else None, _dev(gtex, name="gtex") if gtex is not None else None, float(reg_weight),
               _dev(ws, name="ws") if ws is not None else None, _dev(gd) if gd is not None else None, _dev(gr) if gr is not None else None, _dev(val),
               _dev(loss_in, name="loss_in") if loss_in is not None else None, int(loss_in.numel()) if loss_in is not None else 0, float(loss_div),
               int(ksize), float(blur_sigma), _dev(scratch, name="scratch") if scratch is not None else None, C.byref(adam) if adam is not None else None, _stream())
    return gd, gr, val


_pattern_epochs = {}


_SHARED_STREAMS = {}


def shared_streams(device, role, n):
    """the process's n streams of `role` on `device` (created on first use): every scene / geometry of the device takes the same ones"""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), role)
    got = _SHARED_STREAMS.setdefault(key, [])
    while len(got) < n:
        got.append(torch.cuda.Stream(dev))
    return got[:n]


def pattern_step(rays, KF, sigma, size0, size1, bufs, gtex, reg_weight, ksize, blur_sigma, adam, zero, sync, rays_kept=None, check_kept=False, loss_in=None, loss_div=1.0,
                 epoch=None):
    """The pattern side of a step as ONE launch (ffx_pattern_step): pattern_bwd_blur(..., adam) on `bufs` = (pts, tsum, tsor, ws, tex) of THIS step,
    then — behind the update, in the same launch — pattern_fwd_blur of the NEXT step into the same five tensors, `zero` cleared.
    -> (grays_data, grays_reg, [3] loss values), or None when the library declines the shape (FFX_ERR_UNSUPPORTED: the caller issues the two launches).
    `sync`: uint8 tensor of _abi.PATTERN_SYNC_BYTES, zero before the first call; rays_kept: float32 [2, n, 3]; epoch: 1, 2, 3, ... per launch on this pair of
    buffers (None: counted here)."""
    pts, tsum, tsor, ws, tex = bufs
    n = rays.shape[0]
    gd = torch.empty((n, 3), dtype=torch.float32, device=rays.device) if gtex is not None else None
    gr = torch.empty((n, 3), dtype=torch.float32, device=rays.device) if reg_weight > 0 else None
    val = torch.empty(3, dtype=torch.float32, device=rays.device)
    if sync.numel() < _abi.PATTERN_SYNC_BYTES or sync.dtype != torch.uint8:
        raise ValueError("pattern_step: sync must be a uint8 tensor of PATTERN_SYNC_BYTES")
    if rays_kept is None or rays_kept.numel() != 6 * n:
        raise ValueError("pattern_step: rays_kept must be a float32 tensor [2, n, 3]")
    # the launch's epoch: the caller's count of the launches on this (sync, rays_kept) pair — or, for callers that keep none, a count kept here by the
    # buffers' addresses (a pair that was zeroed and is used again under the same addresses continues the old count: any value but the flags' works)
    key = None
    if epoch is None:
        key = (sync.data_ptr(), rays_kept.data_ptr())
        epoch = _pattern_epochs.get(key, 0) % 0xFFFFFFF0 + 1
        if len(_pattern_epochs) > 256 and key not in _pattern_epochs:
            _pattern_epochs.clear()
    rc = api().call_rc("ffx_pattern_step", _dev(rays, name="rays"), n, _m16(KF), float(sigma), int(size0), int(size1), _dev(tsum, name="tsum"),
                       _dev(tsor, name="tsor") if tsor is not None else None, _dev(gtex, name="gtex") if gtex is not None else None, float(reg_weight),
                       _dev(ws, name="ws") if ws is not None else None, _dev(gd) if gd is not None else None, _dev(gr) if gr is not None else None, _dev(val),
                       _dev(loss_in, name="loss_in") if loss_in is not None else None, int(loss_in.numel()) if loss_in is not None else 0, float(loss_div),
                       int(ksize), float(blur_sigma), C.byref(adam), _dev(pts, name="pts"), _dev(zero, name="zero") if zero is not None else None,
                       int(zero.numel()) if zero is not None else 0, _dev(tex, name="tex"), _dev(rays_kept, name="rays_kept"),
                       int(bool(check_kept)), _dev(sync, torch.uint8, "sync"), epoch, _stream(), allow=(_abi.FFX_ERR_UNSUPPORTED,))
    if rc != 0:
        return None
    if key is not None:
        _pattern_epochs[key] = epoch
    return gd, gr, val


def adam_args(rays, exp_avg, exp_avg_sq, step, counter, lr, beta1, beta2, eps, KF_inv, lo, hi, n_normalize=1, grad_div=1.0, grad_out=None, dot=None, guard=None):
    """ffx_adam_args for pattern_bwd_blur (the tensors must outlive the launch; `counter`: one zeroed int32 / uint32 device word).
    dot = (a, b, partial): the launch also evaluates <a, b> (two float32 tensors of equal size: the render and the constant gradient of a loss
    linear in it) as the step's data term; partial: float32 scratch of one element per point."""
    a = _abi.AdamArgs()
    a.rays = _dev(rays, name="rays").value
    if exp_avg is not None:  # (exp_avg = exp_avg_sq = step = None: no update, only the inner product — a multi-rank step)
        a.exp_avg, a.exp_avg_sq = _dev(exp_avg, name="exp_avg").value, _dev(exp_avg_sq, name="exp_avg_sq").value
        a.step = _dev(step, name="step").value
    a.grad_out = _dev(grad_out, name="grad_out").value if grad_out is not None else None
    a.counter = _dev(counter, torch.int32, "counter").value
    a.lr, a.beta1, a.beta2, a.eps = float(lr), float(beta1), float(beta2), float(eps)
    a.KF_inv = _m16(KF_inv)
    a.lo, a.hi, a.grad_div, a.n_normalize = float(lo), float(hi), float(grad_div), int(n_normalize)
    if dot is not None:
        da, db, part = dot
        if da.numel() % db.numel() != 0 or part.numel() < rays.shape[0]:
            raise ValueError("dot = (a, b, partial): a a whole number of b's long (b is repeated), partial with one float per point")
        a.dot_a, a.dot_b, a.dot_n, a.dot_partial = _dev(da, name="dot a").value, _dev(db, name="dot b").value, int(da.numel()), _dev(part, name="dot partial").value
        a.dot_b_n = int(db.numel())
    if guard is not None:  # an adjoint cache (uint8 tensor): the update is skipped when its header reports dropped samples
        a.guard = _dev(guard, torch.uint8, "guard").value
    # the struct holds raw addresses: it keeps the tensors alive for as long as it lives itself.  (A temporary passed as grad_out used to be
    # freed on return — the caching allocator then handed its block to the NEXT small torch.empty, e.g. pattern_bwd_blur's 3-float value
    # buffer, which the update's gradient store overwrote: an intermittent wrong regulariser value in the test suite, round 4)
    a._keep = (rays, exp_avg, exp_avg_sq, step, counter, grad_out, dot, guard)
    return a


def adam_clamp_step_(rays, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, KF, KF_inv, lo, hi, n_normalize=1, grad_b=None, grad_div=1.0, grad_out=None, guard=None):
    """in place: torch.optim.Adam's update of `rays` followed by Laser.clamp_to_fov + normalisation, one launch.
    With grad_out the gradient used is grad / grad_div + grad_b (stored in grad_out).
    guard: a device tensor (or a slice of one) whose 32-bit word at byte 8 says "skip": an adjoint cache header, or the tail of an
    all-reduced flat buffer (include/ffx.h)."""
    if guard is not None and (not guard.is_cuda or guard.numel() * guard.element_size() < 12):
        raise ValueError("guard must be a device tensor of at least 12 bytes")
    api().call("ffx_adam_clamp_step", _dev(rays, name="rays"), _dev(grad, name="grad"), _dev(grad_b, name="grad_b") if grad_b is not None else None, float(grad_div),
               _dev(grad_out, name="grad_out") if grad_out is not None else None, _dev(exp_avg, name="exp_avg"), _dev(exp_avg_sq, name="exp_avg_sq"),
               _dev(step, name="step"), rays.shape[0], float(lr), float(beta1), float(beta2), float(eps), _m16(KF), _m16(KF_inv), float(lo), float(hi),
               int(n_normalize), guard.data_ptr() if guard is not None else None, _stream())
    return rays


# ------------------------------------------------------------------ K2
def _check_pts(pts):
    if pts.dim() != 2 or pts.shape[1] != 2:
        raise ValueError(f"points must be [N,2], got {tuple(pts.shape)}")


def splat_dense_fwd(pts, sigma, size0, size1):
    _check_pts(pts)
    out = torch.empty((pts.shape[0], size1, size0), dtype=torch.float32, device=pts.device)
    api().call("ffx_splat_dense_fwd", _dev(pts, name="pts"), pts.shape[0], float(sigma), size0, size1, _dev(out), _stream())
    return out


def splat_dense_bwd(pts, sigma, size0, size1, gout):
    _check_pts(pts)
    if tuple(gout.shape) != (pts.shape[0], size1, size0):
        raise ValueError("gout shape mismatch")
    out = torch.empty_like(pts)
    api().call("ffx_splat_dense_bwd", _dev(pts, name="pts"), pts.shape[0], float(sigma), size0, size1, _dev(gout, name="gout"), _dev(out), _stream())
    return out


def splat_fwd(pts, sigma, reduce, half_window, size0, size1):
    _check_pts(pts)
    out = torch.empty((size1, size0), dtype=torch.float32, device=pts.device)
    api().call("ffx_splat_fwd", _dev(pts, name="pts"), pts.shape[0], float(sigma), _reduce(reduce), int(half_window), size0, size1, _dev(out), _stream())
    return out


def splat_bwd(pts, sigma, reduce, half_window, size0, size1, tex, gtex):
    _check_pts(pts)
    if tuple(gtex.shape) != (size1, size0):
        raise ValueError("gtex shape mismatch")
    out = torch.empty_like(pts)
    api().call(
        "ffx_splat_bwd", _dev(pts, name="pts"), pts.shape[0], float(sigma), _reduce(reduce), int(half_window), size0, size1,
        _dev(tex, name="tex") if tex is not None else None, _dev(gtex, name="gtex"), _dev(out), _stream(),
    )
    return out


def splat_depth_fwd(pts, depth, sigma, size0, size1):
    _check_pts(pts)
    depth = depth.reshape(-1)
    out = torch.empty((pts.shape[0], size1, size0), dtype=torch.float32, device=pts.device)
    api().call("ffx_splat_depth_fwd", _dev(pts, name="pts"), _dev(depth, name="depth"), pts.shape[0], float(sigma), size0, size1, _dev(out), _stream())
    return out


def _depth_pair(pts, depth):
    _check_pts(pts)
    depth = depth.reshape(-1)
    if depth.shape[0] != pts.shape[0]:
        raise ValueError(f"depth must hold one value per point: {pts.shape[0]} points, {depth.shape[0]} depths")
    return depth


def splat_depth_bwd(pts, depth, sigma, size0, size1, gout):
    """adjoint of splat_depth_fwd -> (gpts [n,2], gdepth [n])"""
    depth = _depth_pair(pts, depth)
    if tuple(gout.shape) != (pts.shape[0], size1, size0):
        raise ValueError("gout shape mismatch")
    gpts, gdepth = torch.empty_like(pts), torch.empty_like(depth)
    api().call("ffx_splat_depth_bwd", _dev(pts, name="pts"), _dev(depth, name="depth"), pts.shape[0], float(sigma), size0, size1, _dev(gout, name="gout"),
               _dev(gpts), _dev(gdepth), _stream())
    return gpts, gdepth


def splat_depth_softor_fwd(pts, depth, sigma, size0, size1):
    """softor over splat_depth_fwd's layers -> [size1,size0], without the layers"""
    depth = _depth_pair(pts, depth)
    out = torch.empty((size1, size0), dtype=torch.float32, device=pts.device)
    api().call("ffx_splat_depth_softor_fwd", _dev(pts, name="pts"), _dev(depth, name="depth"), pts.shape[0], float(sigma), size0, size1, _dev(out), _stream())
    return out


def splat_depth_softor_bwd(pts, depth, sigma, size0, size1, gout):
    """adjoint of splat_depth_softor_fwd -> (gpts [n,2], gdepth [n])"""
    depth = _depth_pair(pts, depth)
    if tuple(gout.shape) != (size1, size0):
        raise ValueError("gout shape mismatch")
    gpts, gdepth = torch.empty_like(pts), torch.empty_like(depth)
    api().call("ffx_splat_depth_softor_bwd", _dev(pts, name="pts"), _dev(depth, name="depth"), pts.shape[0], float(sigma), size0, size1,
               _dev(gout, name="gout"), _dev(gpts), _dev(gdepth), _stream())
    return gpts, gdepth


def splat_lines_fwd(lines, sigma, size0, size1):
    if lines.dim() != 3 or tuple(lines.shape[1:]) != (2, 2):
        raise ValueError("lines must be [N,2,2]")
    out = torch.empty((lines.shape[0], size1, size0), dtype=torch.float32, device=lines.device)
    api().call("ffx_splat_lines_fwd", _dev(lines, name="lines"), lines.shape[0], float(sigma), size0, size1, _dev(out), _stream())
    return out


def splat_lines_bwd(lines, sigma, size0, size1, gout):
    if tuple(gout.shape) != (lines.shape[0], size1, size0):
        raise ValueError("gout shape mismatch")
    out = torch.empty_like(lines)
    api().call("ffx_splat_lines_bwd", _dev(lines, name="lines"), lines.shape[0], float(sigma), size0, size1, _dev(gout, name="gout"), _dev(out), _stream())
    return out


# ------------------------------------------------------------------ K3
def blur_fwd(img, ksize=5, sigma=3.0):
    if img.dim() != 2:
        raise ValueError("blur expects [H,W]")
    out = torch.empty_like(img)
    api().call("ffx_blur_fwd", _dev(img, name="img"), img.shape[0], img.shape[1], ksize, float(sigma), _dev(out), _stream())
    return out


def silhouette(img, cx, cy, radius, ksize=11, sigma=5.0):
    """img [H,W] times the blurred filled circle of apply_silhouette.py — ffx_silhouette_fwd: blur_fwd(mask) * img bit for bit, one launch, no mask tensor"""
    if img.dim() != 2:
        raise ValueError("silhouette expects [H,W]")
    out = torch.empty_like(img)
    api().call("ffx_silhouette_fwd", _dev(img, name="img"), img.shape[0], img.shape[1], int(cx), int(cy), int(radius), int(ksize), float(sigma), _dev(out), _stream())
    return out


def noise_clamp(img, noise, mean, std, lo=0.0, hi=1.0):
    """clamp(img + (noise * std + mean), lo, hi) in one launch (ffx_noise_clamp); the result takes the noise tensor's place"""
    if img.shape != noise.shape:
        raise ValueError("noise must have the image's shape")
    api().call("ffx_noise_clamp", _dev(img, name="img"), _dev(noise, name="noise"), img.numel(), float(mean), float(std), float(lo), float(hi), _dev(noise), _stream())
    return noise


def rgb_to_gray(img, weights=(0.299, 0.587, 0.114)):
    """[..., 3] float32 / float16 -> [...] float32: (r wr + g wg) + b wb (ffx_rgb_to_gray; cv2.COLOR_RGB2GRAY's weights by default)"""
    if img.shape[-1] != 3 or img.dtype not in (torch.float32, torch.float16):
        raise ValueError("rgb_to_gray expects a [..., 3] float32 or float16 image")
    out = torch.empty(img.shape[:-1], dtype=torch.float32, device=img.device)
    api().call("ffx_rgb_to_gray", _dev(img, img.dtype, "img"), int(img.dtype == torch.float16), out.numel(), float(weights[0]), float(weights[1]), float(weights[2]), _dev(out), _stream())
    return out


class Components(NamedTuple):
    """what connected_components returns, laid out as cv2.connectedComponentsWithStats returns it (include/ffx_labels.h): n_labels — a 0-d
    int32 tensor, components + 1; reading it is the caller's synchronisation —, labels [H, W] int32, stats [max_labels, 5] int32 (left, top, width,
    height, area; row 0 the background), centroids [max_labels, 2] float64 (x, y).  labels / stats and centroids are None where they were not asked for"""
    n_labels: torch.Tensor
    labels: torch.Tensor = None
    stats: torch.Tensor = None
    centroids: torch.Tensor = None


_COMPONENT_DTYPES = {torch.bool: 1, torch.uint8: 1, torch.int32: 4, torch.int64: 8}


def connected_components(img, connectivity=8, background=0, max_labels=256, labels=True, stats=True, workspace=None):
    """The 4- or 8-connected components of the pixels of `img` that differ from `background`, numbered 1..C in raster order of their first pixel, with
    cv2's statistics of the first max_labels labels (ffx_connected_components; main.py:168-180) -> Components.  img: [H, W] bool / uint8 / int32 / int64 on
    a HIP device, contiguous.  labels=False / stats=False skip those outputs and the launches that only serve them.  workspace: a uint8 tensor of at least
    _abi.components_workspace_bytes(H, W, max_labels) bytes to use instead of a fresh one (its contents do not matter)."""
    if not isinstance(img, torch.Tensor):
        raise TypeError("img: expected a torch.Tensor")
    if img.dtype not in _COMPONENT_DTYPES:
        raise TypeError(f"img: expected bool, uint8, int32 or int64, got {img.dtype}")
    if img.dim() != 2:
        raise ValueError(f"img: expected a 2-D image [H, W], got {tuple(img.shape)}")
    if not img.is_contiguous():
        raise ValueError("img: must be contiguous")
    if stats and int(max_labels) < 1:
        raise ValueError(f"max_labels: {max_labels} with stats (at least 1)")
    p_img = _dev(img, img.dtype, "img")
    h, w = int(img.shape[0]), int(img.shape[1])
    need = _abi.components_workspace_bytes(h, w, max_labels if stats else 0)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=img.device)
    elif workspace.numel() < need:
        raise ValueError(f"workspace: {workspace.numel()} bytes, the call needs {need}")
    p_ws = _dev(workspace, torch.uint8, "workspace")
    n = torch.empty((), dtype=torch.int32, device=img.device)
    lab = torch.empty((h, w), dtype=torch.int32, device=img.device) if labels else None
    st = torch.empty((int(max_labels), 5), dtype=torch.int32, device=img.device) if stats else None
    cen = torch.empty((int(max_labels), 2), dtype=torch.float64, device=img.device) if stats else None
    api().call("ffx_connected_components", p_img, _COMPONENT_DTYPES[img.dtype], h, w, int(background), int(connectivity),
               _dev(lab, torch.int32, "labels") if labels else None, _dev(n, torch.int32, "n_labels"), _dev(st, torch.int32, "stats") if stats else None,
               _dev(cen, torch.float64, "centroids") if stats else None, int(max_labels), p_ws, _stream(img.device))
    return Components(n, lab, st, cen)


_PERLIN_LAYOUTS = {"chw": _abi.PERLIN_LAYOUT_CHW, "hwc": _abi.PERLIN_LAYOUT_HWC}


def perlin_angle_count(res, octaves):
    """floats of the packed lattice angles of ffx_perlin_texture: (R0 + 1) * (R1 + 1) per octave, R = res * 2^octave"""
    return sum(((int(res[0]) << o) + 1) * ((int(res[1]) << o) + 1) for o in range(int(octaves)))


def perlin_texture(angles, pos, octaves, res, persistence, shape, color_a, color_b, layout="hwc", workspace=None):
    """color_a .. color_b blended by the normalised multi-octave Perlin noise of DESIGN.md 4.12 (ffx_perlin_texture; main.py:148-153) -> a fresh
    [H, W, 3] (layout "hwc", the renderer's) or [3, H, W] ("chw") float32 tensor.  angles: the octaves' lattice angles packed one after the other,
    perlin_angle_count(res, octaves) floats; pos: per octave the H row positions then the W column positions inside their cells, octaves * (H + W)
    floats; color_a, color_b: [3]; all float32 on one HIP device, contiguous.  workspace: a uint8 tensor of at least _abi.perlin_workspace_bytes(H, W)
    bytes to use instead of a fresh one (its contents do not matter)."""
    for name, t in (("angles", angles), ("pos", pos), ("color_a", color_a), ("color_b", color_b)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch.Tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if layout not in _PERLIN_LAYOUTS:
        raise ValueError(f"layout: {layout!r} ('hwc' or 'chw')")
    octaves, h, w, r0, r1 = int(octaves), int(shape[0]), int(shape[1]), int(res[0]), int(res[1])
    if not 1 <= octaves <= _abi.PERLIN_MAX_OCTAVES:
        raise ValueError(f"octaves: {octaves} outside 1..{_abi.PERLIN_MAX_OCTAVES}")
    if min(h, w, r0, r1) < 1 or max(h, w) > 32768:
        raise ValueError(f"shape / res: {h} x {w} texels (1..32768), a {r0} x {r1} lattice (at least 1 x 1)")
    if (r0 << (octaves - 1)) > h or (r1 << (octaves - 1)) > w:
        raise ValueError(f"res: octave {octaves - 1}'s {r0 << (octaves - 1)} x {r1 << (octaves - 1)} lattice needs at least as many texels per axis (got {h} x {w})")
    if angles.dim() != 1 or angles.numel() != perlin_angle_count((r0, r1), octaves):
        raise ValueError(f"angles: expected {perlin_angle_count((r0, r1), octaves)} packed floats, got {tuple(angles.shape)}")
    if pos.dim() != 1 or pos.numel() != octaves * (h + w):
        raise ValueError(f"pos: expected {octaves * (h + w)} packed floats, got {tuple(pos.shape)}")
    for name, t in (("color_a", color_a), ("color_b", color_b)):
        if tuple(t.shape) != (3,):
            raise ValueError(f"{name}: expected [3], got {tuple(t.shape)}")
    p_ang, p_pos, p_a, p_b = _dev(angles, name="angles"), _dev(pos, name="pos"), _dev(color_a, name="color_a"), _dev(color_b, name="color_b")
    if not angles.device == pos.device == color_a.device == color_b.device:
        raise ValueError("angles, pos, color_a and color_b must live on one device")
    need = _abi.perlin_workspace_bytes(h, w)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=angles.device)
    elif workspace.numel() < need:
        raise ValueError(f"workspace: {workspace.numel()} bytes, the call needs {need}")
    out = torch.empty((h, w, 3) if layout == "hwc" else (3, h, w), dtype=torch.float32, device=angles.device)
    api().call("ffx_perlin_texture", p_ang, p_pos, octaves, r0, r1, float(persistence), h, w, p_a, p_b, _PERLIN_LAYOUTS[layout], _dev(out, name="out"),
               _dev(workspace, torch.uint8, "workspace"), _stream(angles.device))
    return out


def blur_bwd(g, ksize=5, sigma=3.0):
    out = torch.empty_like(g)
    api().call("ffx_blur_bwd", _dev(g, name="g"), g.shape[0], g.shape[1], ksize, float(sigma), _dev(out), _stream())
    return out


def render_cache_bytes(width, height, spp):
    return int(api().lib.ffx_render_cache_bytes(int(width), int(height), int(spp)))


def render_cache_bytes_sd(sd, spp):
    """the adjoint cache of a render of `sd` (larger with material rows: a second footprint per pixel)"""
    return int(api().lib.ffx_render_cache_bytes_sd(C.byref(sd), int(spp)))


def render_filter_bytes(sd):
    """scratch of ffx_render_{fwd,bwd}_filtered for a render of `sd` (400 + 16 bytes per pixel)"""
    return int(api().lib.ffx_render_filter_bytes(C.byref(sd)))


def render_dot_slots(width, height):
    return int(api().lib.ffx_render_dot_slots(int(width), int(height)))


def render_cache_status(cache):
    """(stray records used, arena capacity, dropped samples) of an adjoint cache written by render_fwd(..., cache=...) — for a filtered film's
    cache: (64-sample blocks taken, blocks the arena holds, pixels that found it full and kept no records).
    SYNCHRONISES the current stream (64-byte read).  dropped > 0: the cache is incomplete — ffx_render_bwd_cached then
    poisons gtex[0] with NaN; use the re-tracing adjoint."""
    out = (C.c_uint32 * 3)()
    api().call("ffx_render_cache_status", _dev(cache, torch.uint8, "cache"), out, _stream())
    return int(out[0]), int(out[1]), int(out[2])


_K8_LAUNCHES = None


def k8_launch_counters():
    """The library's two launch counters of the packet render kernel k_render_fwd_pk, read in place: [0] launches of its plain-scene instance,
    [1] of the generic one — which instance the native launcher picked (ffx_trace.hip plain_scene; FFX_K8_PLAIN=0 keeps the generic one).
    Process-wide, never reset: callers take differences.  A build without the symbol (FFX_LIB) reads as zeros."""
    global _K8_LAUNCHES
    if _K8_LAUNCHES is None:
        try:
            _K8_LAUNCHES = (C.c_ulonglong * 2).in_dll(api().lib, "ffx_k8_instance_launches")
        except ValueError:
            _K8_LAUNCHES = (C.c_ulonglong * 2)()
    return _K8_LAUNCHES


def k8_instance_launches():
    """-> (plain-scene, generic) launches so far"""
    k = k8_launch_counters()
    return int(k[0]), int(k[1])


def _check_materials(sd, albedo):
    """-> the pointer argument for shape_albedo: None when the scene description carries the rows itself (sd.n_mat_h)"""
    if sd.n_mat_h > 0:
        return None
    if albedo is None:
        raise ValueError("no material table: pass the device tensor or put the rows into the scene description (scene_desc.set_host_materials)")
    _check_table(sd, albedo)
    return _dev(albedo, name="albedo")


def _check_table(sd, albedo):
    ms = int(sd.mat_stride) or 3
    if albedo.dim() != 2 or albedo.shape[1] != ms or albedo.shape[0] < sd.n_shapes:
        raise ValueError(f"material table {tuple(albedo.shape)} does not match the scene description (n_shapes {sd.n_shapes}, mat_stride {ms})")


# ------------------------------------------------------------------ K5..K9
def camera_struct(to_world, camera_to_sample, near, far, width, height):
    c = _abi.Camera()
    c.to_world = _m16(to_world)
    c.camera_to_sample = _m16(camera_to_sample)
    c.near_clip, c.far_clip, c.width, c.height = float(near), float(far), int(width), int(height)
    return c


class _EventPair:
    """records a HIP event pair on the current stream around one launch (bench.py's live kernel
    timing); a no-op when `sink` is None."""

    def __init__(self, sink, name):
        self.sink, self.name = sink, name

    def __enter__(self):
        if self.sink is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if self.sink is not None:
            self.b.record()
            self.sink.append((self.name, self.a, self.b))
        return False


# the pre-pass knobs are read per call (a test flips them mid-process) — straight from os.environ's own dict where it has one (posix: bytes -> bytes;
# os.environ.get's encode + KeyError path was 0.6 us a look-up, fourteen of them per loop step: a tenth of the host's time at 4 spp)
_ENV_DATA = getattr(os.environ, "_data", None)
_ENV_NAMES = ("FFX_BINS", "FFX_BIN_TILE", "FFX_BIN_TILE_PROJ", "FFX_BIN_SPOT_N", "FFX_BIN_CAP", "FFX_ENVELOPE")
if isinstance(_ENV_DATA, dict) and os.name == "posix":
    _ENV_KEYS = tuple(n.encode() for n in _ENV_NAMES)

    def _apex_env():
        g = _ENV_DATA.get
        return tuple(g(k) for k in _ENV_KEYS)
else:
    def _apex_env():
        g = os.environ.get
        return tuple(g(n) for n in _ENV_NAMES)


def apex_key(sd=None, cam=None):
    """what the blob's pre-pass areas must hold for a packet render / trace call (include/ffx.h ffx_apex_prepare): the apex records depend
    on the POSITIONS of the camera and of the enabled emitters, the tile bins (ffx_bvh_info.off_bins) on their whole projections — pose,
    field of view, film / texture size, the spot's cone — as the exact floats the library reads"""
    if sd is not None:
        k = getattr(sd, "_apex_key", None)  # (a description is never modified once built: mi.Scene makes a new one per pose — 5 us per call otherwise)
        if k is not None and k[1] == _apex_env():
            return k[0]
    c = sd.cam if sd is not None else cam
    # (the structs' bytes: ~1 us each — tuples of their 32 floats were 10 us per render call)
    key = [C.string_at(C.addressof(c), C.sizeof(c))]
    if sd is not None:
        key += [C.string_at(C.addressof(sd.proj), C.sizeof(sd.proj)) if sd.proj.enabled else None]
        # (not the spot's intensity: randomised per step, no part of the pre-pass; `shadows`: the pre-pass builds the envelopes only for a scene that traces shadow rays)
        key += [(C.string_at(C.addressof(sd.spot), 64), sd.spot.cutoff_deg, int(sd.shadows)) if sd.spot.enabled else (None, int(sd.shadows))]
    else:
        key += [None, None]
    env = _apex_env()
    key = tuple(key) + env
    if sd is not None and getattr(sd, "_frozen", False):  # (only descriptions whose maker promises not to touch them again: mi.Scene.scene_desc)
        sd._apex_key = (key, env)
    return key


def _camera_part(key):
    """of an apex_key: what the camera's area (its apex records and tile bins) depends on"""
    return None if key is None else (key[0], key[3], key[4], key[7])  # (camera struct, FFX_BINS, FFX_BIN_TILE, FFX_BIN_CAP)


def deterministic_mode():
    """FFX_DETERMINISTIC=1: every texture gradient comes from ffx_render_bwd_det (64-bit fixed-point accumulation: bitwise reproducible, whatever
    the dispatch order or the number of ranks) instead of the float-atomic adjoints — functional.render's backward and PatternOptimizer.step
    then re-trace.  A cross-checking / debugging mode: two re-traces and one host synchronisation per adjoint."""
    return os.environ.get("FFX_DETERMINISTIC", "0") == "1"


def det_scale_log2(vmax_bits: int, n_taps: int):
    """the power-of-two scale of a deterministic accumulation whose largest |tap| has the float bits `vmax_bits`, over `n_taps` taps in all
    (include/ffx.h ffx_det_scale_log2) — None: nothing lit, or a non-finite tap"""
    sh = int(api().lib.ffx_det_scale_log2(C.c_uint32(int(vmax_bits) & 0xFFFFFFFF), C.c_uint64(int(n_taps))))
    return None if sh < -126 else sh


def det_finish_(acc: torch.Tensor, scale_log2: int, gtex: torch.Tensor):
    """gtex += acc * 2^-scale_log2 (acc: int64 fixed-point sums, one per texel and channel)"""
    if acc.dtype != torch.int64 or not acc.is_contiguous() or gtex.dtype != torch.float32 or not gtex.is_contiguous() or acc.numel() != gtex.numel():
        raise ValueError("det_finish_: int64 sums and a float32 gradient of the same size, both contiguous")
    api().call("ffx_det_finish", C.c_void_p(acc.data_ptr()), int(scale_log2), acc.numel(), C.c_void_p(gtex.data_ptr()), _stream())
    return gtex


def path_flags(max_depth=2, rr_depth=5):
    """the flags bits (include/ffx.h FFX_RENDER_PATH) of a render with Mitsuba's `path` integrator at `max_depth` (2: direct light at the primary hit,
    0 bits — the kernels of every other call; up to 8) with Russian roulette from vertex `rr_depth` on"""
    if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or not 2 <= int(max_depth) <= _abi.RENDER_MAX_DEPTH_LIMIT:
        raise ValueError(f"max_depth must be an integer in 2 .. {_abi.RENDER_MAX_DEPTH_LIMIT} (-1, unbounded, is not served), got {max_depth!r}")
    if isinstance(rr_depth, bool) or not isinstance(rr_depth, (int, np.integer)) or int(rr_depth) < 1:
        raise ValueError(f"rr_depth must be a positive integer, got {rr_depth!r}")
    return _abi.render_path(int(max_depth), min(int(rr_depth), 15))  # (a roulette from vertex 15 on never runs: max_depth <= 8)


def _no_path(max_depth, what):
    if max_depth != 2:
        path_flags(max_depth)  # (the range check's message first)
        raise ValueError(f"{what}: max_depth > 2 renders through render_fwd / render_bwd only (no adjoint cache, fused or deterministic adjoint)")


def pack_lights(lights):
    """the table of a render's extra emitters (include/ffx.h FFX_RENDER_LIGHTS): scenes.LightData entries -> [n, 24] float32 on the host
    (to_world 0..15 row-major, intensity 16..18, cutoff_deg 19, beam_width_deg 20, type 21: 0 point / 1 spot, 22..23 zero; a directional emitter,
    DESIGN.md 4.9: to_world, its irradiance in 16..18, type 2, zeros elsewhere — such a table is rendered with lights_directional=True).  Floats 16..18 are
    what render_bwd(emitters=True) differentiates with respect to: row k of EmitterGrad.lights belongs to record k"""
    lights = list(lights)
    if len(lights) > _abi.RENDER_MAX_LIGHTS:
        raise ValueError(f"at most {_abi.RENDER_MAX_LIGHTS} extra emitters, got {len(lights)}")
    out = torch.zeros((len(lights), _abi.LIGHT_FLOATS), dtype=torch.float32)
    for k, l in enumerate(lights):
        if l.kind not in ("point", "spot", "directional"):
            raise ValueError(f"light {l.name!r}: kind must be 'point', 'spot' or 'directional', got {l.kind!r}")
        out[k, :16] = torch.as_tensor(np.asarray(l.to_world, dtype=np.float32).reshape(16))
        out[k, 16:19] = torch.as_tensor([float(v) for v in l.intensity], dtype=torch.float32)
        if l.kind == "directional":
            out[k, 21] = float(_abi.LIGHT_DIRECTIONAL)
            continue
        out[k, 19], out[k, 20] = float(l.cutoff_angle), float(l.beam_width)
        out[k, 21] = float(_abi.LIGHT_SPOT if l.kind == "spot" else _abi.LIGHT_POINT)
    return out


def lights_directional(lights):
    """whether a list of scenes.LightData holds a directional emitter: the lights_directional= of the render that takes pack_lights(lights)"""
    return any(l.kind == "directional" for l in lights)


def pack_ambient(ambient):
    """a render's ambient record (include/ffx.h FFX_RENDER_AMBIENT): three floats, a [3] tensor or a scenes.AmbientData -> [4] float32
    (radiance r, g, b and a reserved 0) on the tensor's device (the host otherwise); None stays None"""
    if ambient is None:
        return None
    rad = getattr(ambient, "radiance", ambient)
    t = rad.detach().to(torch.float32).reshape(-1) if isinstance(rad, torch.Tensor) else torch.tensor([float(v) for v in rad], dtype=torch.float32)
    if t.numel() != 3:
        raise ValueError(f"ambient: a radiance of three floats, got {t.numel()}")
    return torch.cat([t, t.new_zeros(_abi.AMBIENT_FLOATS - 3)])


# the block of render_aov (include/ffx.h FFX_RENDER_AOV): channel -> (first float, floats), in the block's order
AOV_CHANNELS = {"depth": (0, 1), "position": (1, 3), "geo_normal": (4, 3), "sh_normal": (7, 3), "uv": (10, 2), "albedo": (12, 3), "shape_index": (15, 1),
                "prim_index": (16, 1)}
assert sum(n for _, n in AOV_CHANNELS.values()) == _abi.RENDER_AOV_FLOATS


class AppearanceGrad(NamedTuple):
    """what render_bwd(..., appearance=True) adds to the texture gradient: d loss / d base colour per material row [n_shapes, 3] (zero on
    rows whose base colour is a texture), d loss / d spot intensity [3], d loss / d base-colour texture [h, w, 3] per texture of the scene description.
    material (render_bwd(..., material=True), FFX_RENDER_GRAD_MATERIAL): d loss / d the BSDF parameters per material row [n_shapes, 11], columns
    roughness .. clearcoat_gloss in scenes.MAT_COLUMN order (the eta column: d loss / d eta; at eta = 1 the limit include/ffx.h describes); else None"""
    rows: torch.Tensor
    spot: torch.Tensor
    base_tex: list
    material: torch.Tensor = None


def appearance_blocks(sd, material, buf, start):
    """the gradient / tangent blocks of a render of `sd` (include/ffx.h: [n_shapes][3] rows, [3] spot, [h][w][3] per base-colour texture, then — with
    `material` — [n_shapes][11]) as views into the flat float buffer `buf` from float `start` on: the one place that knows their order and offsets
    -> (an AppearanceGrad of the views, the floats they cover: _abi.appearance_floats [+ _abi.material_floats])"""
    S, o = int(sd.n_shapes), int(start)
    shapes = [(S, 3), (3,)] + [(int(sd.base_tex_h[k]), int(sd.base_tex_w[k]), 3) for k in range(sd.n_base_tex)] + [(S, _abi.RENDER_MATERIAL_COLS)] * bool(material)
    views = []
    for shape in shapes:
        n = math.prod(shape)
        views.append(buf[o:o + n].view(shape))
        o += n
    mat = views.pop() if material else None
    return AppearanceGrad(views[0], views[1], views[2:], mat), o - int(start)


class EmitterGrad(NamedTuple):
    """what render_bwd(..., emitters=True) adds to the texture gradient (FFX_RENDER_EMITTER_GRAD): lights [n, 3] — d loss / d (the RGB power
    of record k of the `lights` table: floats 16..18, a point light's or spot's intensity, a directional emitter's irradiance) — and ambient [3], d loss /
    d (the constant emitter's radiance), None for a call without `ambient`"""
    lights: torch.Tensor
    ambient: torch.Tensor = None


# what a render entry point does about a film with a reconstruction filter (sd.rfilter): DeviceGeometry._launch
_TWIN, _SLOT, _OWN = 0, 1, 2


def _lane_kernels():
    return os.environ.get("FFX_TRAVERSAL") == "lane"  # (the per-lane A/B kernels neither read nor write apex records)


class DeviceGeometry:
    """Triangle soup + BVH blob resident in HBM.

    src_verts [P,3] : vertex pool (all shapes, all animation frames)
    tris [F,3]      : shape-local vertex indices
    tri_shape [F]   : shape id per triangle
    vert_off [S]    : pool offset of each shape's current frame
    The topology is built once on the host (ffx_bvh_build_host) from `build_verts` (defaults to the
    pool at the given offsets); `update()` is the per-randomisation device pass (K5+K6).
    """

    def __init__(self, src_verts, tris, tri_shape, vert_off, device="cuda", build_xforms=None, smooth=None):
        """smooth: one flag per shape — interpolated shading normals, re-derived from the posed vertices by every update()
        (include/ffx.h ffx_smooth: what Mitsuba does for meshes that carry vertex normals)."""
        src = np.ascontiguousarray(src_verts, dtype=np.float32).reshape(-1, 3)
        tr = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
        ts = np.ascontiguousarray(tri_shape, dtype=np.int32).reshape(-1)
        vo = np.ascontiguousarray(vert_off, dtype=np.int32).reshape(-1)
        F, S = tr.shape[0], vo.shape[0]
        if ts.shape[0] != F:
            raise ValueError("tri_shape must have one entry per triangle")
        if F < 1 or S < 1:
            raise ValueError("need at least one triangle and one shape")
        if ts.min() < 0 or ts.max() >= S:
            raise ValueError("tri_shape out of range")
        if tr.min() < 0:
            raise ValueError("negative vertex index")
        self.n_tris, self.n_shapes = F, S
        self.device = torch.device(device)
        self._didx = _dev_index(self.device) if self.device.type == "cuda" and torch.cuda.is_available() else None
        self.timing = None  # set to a list to collect (name, start_event, end_event) per launch
        self._max_local = np.zeros(S, np.int64)
        np.maximum.at(self._max_local, ts, tr.max(axis=1))
        self._pool_size = src.shape[0]
        self._check_offsets(vo)
        # host build from the pose given by the current offsets (+ optional per-shape transforms)
        glob = (tr + vo[ts][:, None]).astype(np.int32)
        bverts = src
        if build_xforms is not None:
            bx = np.asarray(build_xforms, dtype=np.float32).reshape(S, 4, 4)
            bverts = src.copy()
            used = np.unique(glob)
            owner = np.zeros(src.shape[0], np.int64)
            owner[glob.reshape(-1)] = np.repeat(ts, 3)
            v = src[used]
            m = bx[owner[used]]
            bverts[used] = np.einsum("nij,nj->ni", m[:, :3, :3], v) + m[:, :3, 3]
        a = api()
        nbytes = a.lib.ffx_bvh_blob_bytes(F)
        blob = np.zeros(nbytes, np.uint8)
        self.info = _abi.BvhInfo()
        a.call("ffx_bvh_build_host", bverts.ctypes.data, bverts.shape[0], glob.ctypes.data, F, blob.ctypes.data, nbytes, C.byref(self.info))
        # Two copies of the blob: update() re-fits the one that is NOT being read, on a side stream, while
        # the render kernels of the previous step are still running on the caller's stream (the refit is
        # five small dependent launches, ~55 us with the GPU otherwise idle; overlapped it costs nothing).
        # FFX_ASYNC_UPDATE=0 falls back to one blob, everything on the caller's stream.
        # the host builder fills the first off_bins bytes; the tail (tile bins, apex records) is scratch of the render calls' pre-pass
        static = int(self.info.off_bins) if int(self.info.off_bins) > 0 else int(self.info.total_bytes)
        b0 = torch.zeros(int(self.info.total_bytes), dtype=torch.uint8, device=self.device)
        b0[:static].copy_(torch.from_numpy(blob[:static]))
        self._async = self.device.type == "cuda" and os.environ.get("FFX_ASYNC_UPDATE", "1") != "0"
        # (round 5: four copies, of which renders at 33 samples per pixel and more use two — see _ring)
        n_copies = 4 if self._async else 1
        self._blobs = [b0] + [b0.clone() for _ in range(n_copies - 1)]
        self._cur = 0
        # (the side stream has the default priority: a high-priority queue left renders/s unchanged and took gradient steps 2 130 -> 1 540 per
        # second — the step's small launches on the main stream then wait behind it)
        # (round 6: ONE side stream — and one pair of render streams, shared_streams below — per device and process, not per geometry: the streams of a
        # scene that was used a moment ago keep their hardware queues, and a second scene's own streams then share what is left — its consecutive renders
        # lost their overlap: configs[4] behind a two-stream bracket of the vocal fold, 125 -> 118 renders/s, K8 alone unchanged)
        self._side = shared_streams(self.device, "side", 1)[0] if self._async else None
        self._side_handles = {}
        self._last_spp = 64  # samples per pixel of the last render call (how deep update() lets the poses run ahead: _ring)
        self._upd_done = [None] * n_copies   # event: the refit of blob i has been enqueued up to here (side stream)
        self._top = [None] * n_copies        # the top of blob i's tree: None = in place; True = owed (FFX_STEP_DEFER_TOP); a stream handle = launched there (_top_ev)
        self._top_ev = [None] * n_copies
        # (measured, 100-step render loops of the vocal fold: 1 / 4 / 8 spp +11 / +17 / +16 % with the top deferred, 10 / 12 / 16 spp -4 / -2 / -4 %, 64 spp
        # unchanged — a render of a few samples waits for the chain, a longer one for the GPU, where the extra launch in front of it only costs: deferred
        # while the last render had at most FFX_DEFER_TOP samples per pixel, default 8; 0: never)
        self._defer_top_spp = int(os.environ.get("FFX_DEFER_TOP", "8"))
        self._apex = [None] * n_copies       # apex_key of what blob i's apex areas hold (None: nothing usable)
        self._apex_written = [None] * n_copies  # (stream handle, event) behind the call whose own pre-pass last wrote blob i's apex areas
        self._apex_writer_pending = False
        self._last_use = [{} for _ in range(n_copies)]       # per blob: stream handle -> event behind that stream's last reader (renders may come from several streams)
        self.src_verts = torch.from_numpy(src).to(self.device)
        self.tris = torch.from_numpy(tr).to(self.device)
        self.tri_shape = torch.from_numpy(ts).to(self.device)
        self.vert_off = torch.from_numpy(vo).to(self.device)
        self._vert_off_host = vo.copy()
        self._vert_off_dev_stale = False
        self._pool_written = None  # event: the last write_verts() into the vertex pool (caller's stream)
        self.version = 0           # bumped by every update(): functional._Render pins the pose it traced
        self._smooth = None
        if smooth is not None and any(smooth):
            from . import scenes as _scenes

            if S > 32:
                raise NotImplementedError("interpolated normals: at most 32 shapes (the per-shape tables travel as kernel arguments)")
            flags, vbase, a0, adj, n_vn = _scenes.smooth_tables(tr, ts, smooth, S)
            keep = {"flags": np.ascontiguousarray(flags), "vbase": np.ascontiguousarray(vbase), "adj_start": torch.from_numpy(a0).to(self.device),
                    "adj": torch.from_numpy(adj if adj.size else np.zeros(1, np.int32)).to(self.device),
                    "vn": torch.zeros((n_vn, 3), dtype=torch.float32, device=self.device)}  # scratch of the update (side stream)
            sm = _abi.Smooth()
            sm.shape_smooth = keep["flags"].ctypes.data_as(C.POINTER(C.c_int32))
            sm.shape_vbase = keep["vbase"].ctypes.data_as(C.POINTER(C.c_int32))
            sm.adj_start, sm.adj, sm.n_vn, sm.vnormals = keep["adj_start"].data_ptr(), keep["adj"].data_ptr(), int(n_vn), keep["vn"].data_ptr()
            self._smooth = (sm, keep)
        self.smooth = [bool(f) for f in smooth] if smooth is not None else [False] * S
        if self._async:  # blob copies / uploads above were enqueued on the caller's stream
            self._side.wait_stream(_stream_obj(self._didx))
        self.update(torch.eye(4, dtype=torch.float32).repeat(S, 1, 1) if build_xforms is None else torch.from_numpy(np.asarray(build_xforms, np.float32)))

    @property
    def blob(self):
        """the blob the next render / trace call will read (ordered after its refit on the current stream)"""
        self._acquire()
        return self._blobs[self._cur]

    def _acquire(self):
        ev = self._upd_done[self._cur] if self._async else None
        if ev is not None:
            _stream_obj(self._didx).wait_event(ev)
        if self._async:
            # (round 6) a natively pushed pose leaves the TOP of its tree to the first call that walks it (FFX_STEP_DEFER_TOP: the chain a short render
            # waits for is one dependent launch shorter; the top — one workgroup — runs here, on the reader's own stream, beside the previous render).
            # A second reader on another stream waits for that launch.
            i = self._cur
            tp = self._top[i]
            if tp is True:
                so = _stream_obj(self._didx)
                self._call("ffx_scene_refit_top", _dev(self._blobs[i], torch.uint8, "blob"), C.byref(self.info), _stream(self._didx))
                e = self._top_ev[i]
                if e is None:
                    e = self._top_ev[i] = torch.cuda.Event()
                e.record(so)
                self._top[i] = so.cuda_stream
            elif tp is not None:
                so = _stream_obj(self._didx)
                if tp != so.cuda_stream:
                    so.wait_event(self._top_ev[i])

    def _release(self):
        if self.device.type == "cuda":
            so = _stream_obj(self._didx)
            d = self._last_use[self._cur if self._async else 0]
            ev = d.get(so.cuda_stream)
            if ev is None:
                ev = d[so.cuda_stream] = torch.cuda.Event()
            ev.record(so)
            if self._apex_writer_pending:  # this call wrote the apex areas itself: a render on ANOTHER stream that finds them "ready" waits for it
                self._apex_written[self._cur if self._async else 0] = (so.cuda_stream, ev)
                self._apex_writer_pending = False

    def _ring(self):
        """how many of the blob copies the next update() rotates through.  A render at 64 spp (0.39 ms) hides the whole side chain of the next pose
        (re-fit -> count -> scan -> fill, ~0.18 ms beside it) behind itself with two copies — more only cost (2 050 / 2 043 / 2 038 renders/s with 2 / 3 / 4).
        Below 33 spp the render is as short as the chain, and with two copies the chain of pose i + 2 has to wait for the render of pose i: 5 435 /
        5 735 / 6 002 renders/s at 1 spp, 5 107 / 5 384 / 5 602 at 10 spp with 2 / 3 / 4 copies."""
        n = len(self._blobs)
        return n if self._last_spp <= 32 else min(n, 2)

    def _wait_readers(self, i, stream_obj):
        """`stream_obj` is about to WRITE into blob i (a re-fit, an apex pre-pass): every reader on another stream must be done"""
        for handle, ev in self._last_use[i].items():
            if handle != stream_obj.cuda_stream:
                stream_obj.wait_event(ev)

    def write_verts(self, offset, verts):
        """copy caller-supplied vertices [V,3] into the pool at `offset` (animation functions, direct
        `vertex_positions` assignment).  Ordered against the refits on the side stream in both
        directions: the copy waits for every enqueued refit (one may still be reading this slot), and
        the next update() waits for the copy."""
        main = _stream_obj(self._didx)
        if self._async:
            for ev in self._upd_done:
                if ev is not None:
                    main.wait_event(ev)
        self.src_verts[offset : offset + verts.shape[0]].copy_(verts)
        if self._async:
            if self._pool_written is None:
                self._pool_written = torch.cuda.Event()
            self._pool_written.record(main)

    def _call(self, name, *args):
        """a launch on this geometry's device (which need not be the current one)"""
        if self.device.index is None or torch._C._cuda_getDevice() == self.device.index:
            return api().call(name, *args)
        with torch.cuda.device(self.device):
            return api().call(name, *args)

    def _check_offsets(self, vo):
        if (vo < 0).any() or ((vo.astype(np.int64) + self._max_local) >= self._pool_size).any():
            raise ValueError("vert_off + triangle index exceeds the vertex pool")

    def update(self, xforms, vert_off=None, apex_sd=None):
        """K5+K6.  xforms [S,4,4]; optional new frame offsets [S] (host ints).
        apex_sd: the scene description the next renders will use — its apex records are written right behind the re-fit (on the
        side stream, off the renders' critical path) and those renders are told FFX_RENDER_APEX_READY.
        Host xforms (CPU tensor / ndarray) with S <= 32 go through ffx_scene_update_h: the tables
        are kernel arguments, nothing is copied to the device and the call never blocks.  A device
        tensor of xforms uses ffx_scene_update (device-resident randomisers)."""
        if vert_off is not None:
            vo = np.ascontiguousarray(vert_off, dtype=np.int32).reshape(-1)
            if vo.shape[0] != self.n_shapes:
                raise ValueError("vert_off must have one entry per shape")
            self._check_offsets(vo)
            self._vert_off_host = vo.copy()
            self._vert_off_dev_stale = True
        on_device = isinstance(xforms, torch.Tensor) and xforms.is_cuda
        self.version += 1
        if not self._async:
            if self.device.type == "cuda":
                self._wait_readers(0, _stream_obj(self._didx))
            self._update_into(self._blobs[0], xforms, on_device)
            self._prepare_apex(0, apex_sd)
            return
        nxt = (self._cur + 1) % self._ring()
        main = _stream_obj(self._didx)
        side = self._side
        self._wait_readers(nxt, side)  # its readers must be done before it is overwritten
        if self._pool_written is not None:
            side.wait_event(self._pool_written)  # caller-supplied vertices must have landed in the pool
        if on_device:
            side.wait_stream(main)  # the tables were produced on the caller's stream
            xforms.record_stream(side)
        ev = self._upd_done[nxt]
        if ev is None:
            ev = self._upd_done[nxt] = torch.cuda.Event()
        self._top[nxt] = None  # (this path re-fits the whole tree)
        if self.timing is None and not on_device:
            # (the two launch calls take the side stream's handle as an argument: making it the current stream first — a context manager and
            # two current-stream queries — cost 10 us of the 65 this method took per step; the timed / device-table paths keep that form)
            sh = self._side_handle_of(side)
            self._update_into(self._blobs[nxt], xforms, on_device, sh)
            self._prepare_apex(nxt, apex_sd, sh)
            ev.record(side)
        else:
            with torch.cuda.stream(side):
                self._update_into(self._blobs[nxt], xforms, on_device)
                self._prepare_apex(nxt, apex_sd)
                ev.record(side)
        self._cur = nxt

    def _side_handle_of(self, side):
        h = self._side_handles.get(side.cuda_stream)
        if h is None:
            h = self._side_handles[side.cuda_stream] = C.c_void_p(side.cuda_stream)
        return h

    def update_native(self, launch, vert_off):
        """update() for a caller whose ONE native call enqueues the re-fit and the pre-pass (mi.Scene.step_native -> ffx_scene_step_h):
        the same blob rotation and ordering.  launch(blob index, side stream handle, with the pre-pass?) -> the scene description whose apex records and
        tile bins the blob then holds; vert_off: the frame offsets [S] the call used (host int32, already checked by it)."""
        self.version += 1
        nxt = (self._cur + 1) % self._ring()
        side = self._side
        self._wait_readers(nxt, side)
        if self._pool_written is not None:
            side.wait_event(self._pool_written)
        ev = self._upd_done[nxt]
        if ev is None:
            ev = self._upd_done[nxt] = torch.cuda.Event()
        sh = self._side_handle_of(side)
        self._apex[nxt] = None
        self._apex_written[nxt] = None
        self._top[nxt] = None
        if self.timing is None:
            defer = self._last_spp <= self._defer_top_spp
            sd = launch(nxt, sh, 3 if defer else 1)  # (bit 1: FFX_STEP_DEFER_TOP — _acquire launches the top in front of the first reader)
            if defer:
                self._top[nxt] = True
            self._apex[nxt] = apex_key(sd)
        else:  # (bench.py's per-launch event pairs: around the re-fit alone, as on the Python path; the pre-pass as a call of its own behind them)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(side)
            sd = launch(nxt, sh, 0)
            b.record(side)
            self.timing.append(("scene_update", a, b))
            self._prepare_apex(nxt, sd, sh)
        np.copyto(self._vert_off_host, vert_off)
        self._vert_off_dev_stale = True
        ev.record(side)
        self._cur = nxt

    def _prepare_apex(self, i, sd, stream=None):
        """(on the stream the re-fit of blob i was enqueued on) the records changed: what the apex areas held is void"""
        self._apex[i] = None
        self._apex_written[i] = None
        if sd is not None and not _lane_kernels():
            self._call("ffx_apex_prepare", _dev(self._blobs[i], torch.uint8, "blob"), C.byref(self.info), C.byref(sd), stream if stream is not None else _stream(self._didx))
            self._apex[i] = apex_key(sd)

    def _apex_flag(self, key):
        """FFX_RENDER_APEX_READY if the current blob's apex areas hold `key`; they will after the call either way"""
        i = self._cur if self._async else 0
        ready = self._apex[i] == key and not _lane_kernels()
        if self.device.type == "cuda":
            so = _stream_obj(self._didx)
            if not ready:
                self._wait_readers(i, so)  # the call's pre-pass rewrites the apex areas: renders on other streams may still read them
                self._apex_writer_pending = True
            else:
                w = self._apex_written[i]
                if w is not None and w[0] != so.cuda_stream:
                    so.wait_event(w[1])  # written by a pre-pass on another stream (not by the re-fit, which _acquire has waited for)
        if _lane_kernels():
            self._apex[i] = None  # (a cache-writing render runs the packet kernel — and its pre-pass — even then: claim nothing afterwards)
            return 0
        self._apex[i] = key
        return _abi.RENDER_APEX_READY if ready else 0

    def _update_into(self, blob, xforms, on_device, stream=None):
        with self._timed("scene_update"):
            if not on_device and self.n_shapes <= 32:
                xf = xforms.detach().numpy() if isinstance(xforms, torch.Tensor) else np.asarray(xforms)
                # the host tables go through two persistent ctypes arrays with numpy views on them: `ndarray.ctypes.data_as`
                # per call cost more than the launch it fed (measured 120 us each inside the optimiser's loop)
                tabs = getattr(self, "_host_tabs", None)
                if tabs is None:
                    xc, oc = (C.c_float * (16 * self.n_shapes))(), (C.c_int32 * self.n_shapes)()
                    tabs = self._host_tabs = (xc, np.frombuffer(xc, dtype=np.float32).reshape(self.n_shapes, 16), oc, np.frombuffer(oc, dtype=np.int32))
                tabs[1][...] = np.asarray(xf, dtype=np.float32).reshape(self.n_shapes, 16)
                tabs[3][...] = self._vert_off_host
                self._call(
                    "ffx_scene_update_h", _dev(blob, torch.uint8, "blob"), C.byref(self.info), _dev(self.src_verts), _dev(self.tris, torch.int32),
                    _dev(self.tri_shape, torch.int32), tabs[2], tabs[0], self.n_shapes, C.byref(self._smooth[0]) if self._smooth is not None else None,
                    stream if stream is not None else _stream(self._didx),
                )
                return
            if self._vert_off_dev_stale:
                self.vert_off = torch.from_numpy(self._vert_off_host).to(self.device)
                self._vert_off_dev_stale = False
            xf = xforms if isinstance(xforms, torch.Tensor) else torch.as_tensor(np.asarray(xforms, np.float32))
            xf = xf.to(device=self.device, dtype=torch.float32).reshape(self.n_shapes, 16).contiguous()
            self._xf = xf  # keep alive until the stream has consumed it
            self._call(
                "ffx_scene_update", _dev(blob, torch.uint8, "blob"), C.byref(self.info), _dev(self.src_verts), _dev(self.tris, torch.int32),
                _dev(self.tri_shape, torch.int32), _dev(self.vert_off, torch.int32), _dev(xf), self.n_shapes,
                C.byref(self._smooth[0]) if self._smooth is not None else None, _stream(self._didx),
            )

    def trace_primary(self, cam, spp=1, jitter=0, seed=0, want_ids=True):
        n = cam.width * cam.height * spp
        t = torch.empty(n, dtype=torch.float32, device=self.device)
        shape = torch.empty(n, dtype=torch.int32, device=self.device) if want_ids else None
        prim = torch.empty(n, dtype=torch.int32, device=self.device) if want_ids else None
        flags = 0
        if not _lane_kernels():
            i = self._cur if self._async else 0
            self._acquire()
            so = _stream_obj(self._didx)
            key = apex_key(cam=cam)
            if _camera_part(self._apex[i]) == _camera_part(key):
                # the camera's area already holds this camera's records and tile bins (a render of this pose from it, or an earlier trace):
                # nothing is rewritten — whatever the areas were claimed to hold, they still do
                flags = _abi.RENDER_APEX_READY
                w = self._apex_written[i]
                if w is not None and w[0] != so.cuda_stream:
                    so.wait_event(w[1])
            else:
                self._apex[i] = key  # (it rewrites the camera's area; the emitters' areas keep what they had, but a render has to re-derive its own)
                self._wait_readers(i, so)
                self._apex_writer_pending = True
        self._call(
            "ffx_trace_primary", _dev(self.blob, torch.uint8), C.byref(self.info), C.byref(cam), int(spp), int(bool(jitter)) | flags, int(seed) & 0xFFFFFFFF,
            _dev(t), _dev(shape, torch.int32) if want_ids else None, _dev(prim, torch.int32) if want_ids else None, _stream(self._didx),
        )
        self._release()
        return t, shape, prim

    def trace_rays(self, origins, dirs, tmax=3.0e38):
        n = origins.shape[0]
        t = torch.empty(n, dtype=torch.float32, device=self.device)
        shape = torch.empty(n, dtype=torch.int32, device=self.device)
        prim = torch.empty(n, dtype=torch.int32, device=self.device)
        self._call(
            "ffx_trace_rays", _dev(self.blob, torch.uint8), C.byref(self.info), _dev(origins, name="origins"), _dev(dirs, name="dirs"), n, float(tmax),
            _dev(t), _dev(shape, torch.int32), _dev(prim, torch.int32), _stream(self._didx),
        )
        self._release()
        return t, shape, prim

    def trace_rays_bwd(self, origins, dirs, t, prim, gt):
        """adjoint of trace_rays's t with respect to the rays on the pose the forward traced -> (gorig [n,3], gdir [n,3])"""
        n = origins.shape[0]
        gorig, gdir = torch.empty_like(origins), torch.empty_like(dirs)
        self._call(
            "ffx_trace_rays_bwd", _dev(self.blob, torch.uint8), C.byref(self.info), _dev(origins, name="origins"), _dev(dirs, name="dirs"), n,
            _dev(t, name="t"), _dev(prim, torch.int32, "prim"), _dev(gt, name="gt"), _dev(gorig), _dev(gdir), _stream(self._didx),
        )
        self._release()
        return gorig, gdir

    def _timed(self, name):
        return _EventPair(self.timing, name)

    def _with_lights(self, sd, albedo, mats_arg, lights, what, ambient=None, lights_directional=False):
        """a call's extra emitters (include/ffx.h FFX_RENDER_LIGHTS): -> (the shape_albedo argument, the flags bits, the buffer to keep alive).  lights:
        None / empty — the call as it was; else a [n, 24] float32 device tensor (pack_lights), which travels behind the material table in one buffer
        [table | lights] (a scene description that carries its rows: their area is there but not read).  ambient (FFX_RENDER_AMBIENT):
        three floats or a [3] tensor — its record stands behind the lights, [table | lights | ambient], with or without lights.  lights_directional
        (FFX_RENDER_LIGHTS_DIRECTIONAL): the table may hold directional records; without a table the bit is not set"""
        amb = pack_ambient(ambient)
        if lights is not None and lights.numel() == 0:
            lights = None
        if lights is None and amb is None:
            return mats_arg, 0, None
        if lights is None:
            lights = torch.zeros((0, _abi.LIGHT_FLOATS), dtype=torch.float32, device=self.device)
        if lights.dim() != 2 or lights.shape[1] != _abi.LIGHT_FLOATS or lights.dtype != torch.float32:
            raise ValueError(f"{what}: lights must be a [n, {_abi.LIGHT_FLOATS}] float32 tensor (ops.pack_lights)")
        n = int(lights.shape[0])
        if n > _abi.RENDER_MAX_LIGHTS:
            raise ValueError(f"{what}: at most {_abi.RENDER_MAX_LIGHTS} extra emitters, got {n}")
        ms = max(int(sd.mat_stride), 3)
        S = int(sd.n_shapes)
        if albedo is not None:
            _check_table(sd, albedo)
            rows = albedo[:S].detach().to(device=self.device, dtype=torch.float32).reshape(-1)
        else:
            rows = torch.zeros(S * ms, dtype=torch.float32, device=self.device)
        parts = [rows, lights.detach().to(self.device).reshape(-1)] + ([amb.to(self.device)] if amb is not None else [])
        buf = torch.cat(parts).contiguous()
        if ms == _abi.MAT_STRIDE and buf.data_ptr() % 16:
            raise ValueError(f"{what}: the [table | lights] buffer is not 16-byte aligned")
        bits = _abi.render_lights(n) | (_abi.RENDER_AMBIENT if amb is not None else 0) | (_abi.RENDER_LIGHTS_DIRECTIONAL if lights_directional and n else 0)
        return _dev(buf, name="albedo"), bits, buf

    def _launch(self, timer, name, film, blob, sd, lead, spp, seed, flags, *rest):
        """every render call that reads a blob: `name`(blob, info, sd, *lead, spp, seed, flags, *rest, [scratch,] stream) inside the `timer` bracket, then
        the release.  lead: (materials,) for the adjoints, (materials, texture) for the forwards.  film: what `name` does about a film with a
        reconstruction filter (sd.rfilter) — _TWIN: name + "_filtered" serves it and takes a scratch tensor in front of the stream; _SLOT: `name`
        serves both films and always has that argument, None for a box film; _OWN: `name` serves both films from the arguments the caller gives"""
        if film != _OWN and sd.rfilter:
            if film == _TWIN:
                name += "_filtered"
            # (caching allocator, stream-ordered: renders on two streams never share one)
            rest += (_dev(torch.empty(render_filter_bytes(sd), dtype=torch.uint8, device=self.device), torch.uint8),)
        elif film == _SLOT:
            rest += (None,)
        with self._timed(timer):
            self._call(name, _dev(blob, torch.uint8), C.byref(self.info), C.byref(sd), *lead, int(spp), int(seed) & 0xFFFFFFFF, flags, *rest, _stream(self._didx))
        self._release()

    def _launch_fwd(self, timer, blob, sd, mats_arg, tex_arg, spp, seed, flags, img_arg):
        """ffx_render_fwd[_filtered]: the render (render_fwd: direct light or path bits) and, with FFX_RENDER_TANGENT, the forward mode (render_jvp)"""
        self._launch(timer, "ffx_render_fwd", _TWIN, blob, sd, (mats_arg, tex_arg), spp, seed, flags, img_arg)

    def _launch_bwd(self, blob, sd, mats_arg, spp, seed, flags, gimg_arg, gtex_arg):
        """ffx_render_bwd[_filtered]: the re-tracing adjoint (render_bwd: direct light or path bits) and, with FFX_RENDER_GRAD_APPEARANCE, the one that
        also yields the appearance blocks (_render_bwd_leaves)"""
        self._launch("render_bwd", "ffx_render_bwd", _TWIN, blob, sd, (mats_arg,), spp, seed, flags, gimg_arg, gtex_arg)

    def render_fwd(self, sd, albedo, tex, spp, seed=0, fp16=False, cache=None, sparse_adjoint=False, cache_zeroed=False, keep_dropped=False, img_out=None,
                   max_depth=2, rr_depth=5, lights=None, ambient=None, lights_directional=False):
        """K8.  With `cache` (a uint8 tensor of render_cache_bytes(...) bytes) the kernel also stores one
        footprint of every pixel in the projector texture for render_bwd_cached (opaque layout, ffx.h).
        sparse_adjoint (with a cache): FFX_RENDER_SPARSE_ADJOINT — gradients are only wanted at texels whose value is
        not zero (a pattern optimiser's case), dark footprints are skipped.  cache_zeroed: FFX_RENDER_CACHE_ZEROED — the caller has
        cleared the first 64 bytes of `cache` on this stream.  keep_dropped: FFX_RENDER_CACHE_KEEP_DROPPED — the header's count of dropped
        samples survives this call's reset (the later scene samples of a step that reuses one cache).
        A filtered film (sd.rfilter) with a cache: ffx_render_fwd_cache_filtered (per-sample records; render_bwd_cached needs the seed).
        max_depth > 2: Mitsuba's `path` integrator — no cache; its adjoint is render_bwd with the same max_depth / rr_depth / seed.
        lights: a [n, 24] float32 device tensor of extra emitters (pack_lights) — the image of the call without them plus each light's own
        part, at direct light and under max_depth > 2, on either film; fp32 film, no cache.
        ambient: the constant emitter's radiance (three floats or a [3] tensor) — as lights: added to the image by the same pass, fp32
        film, no cache.
        lights_directional: the table may hold directional emitters (ops.lights_directional(the list) tells) — the pass's kernels that
        know all three record types; a table without such a record renders the same image either way."""
        path = path_flags(max_depth, rr_depth) if max_depth != 2 else 0
        if path and cache is not None:
            raise ValueError("render_fwd: max_depth > 2 has no adjoint cache (its adjoint is render_bwd with the same max_depth)")
        if lights is not None and lights.numel() and (fp16 or cache is not None):
            raise ValueError("render_fwd: extra emitters (lights=) are served on the fp32 film without an adjoint cache")
        if ambient is not None and (fp16 or cache is not None):
            raise ValueError("render_fwd: the constant emitter (ambient=) is served on the fp32 film without an adjoint cache")
        H, W = sd.cam.height, sd.cam.width
        self._last_spp = spp
        mats_arg = _check_materials(sd, albedo)
        img = torch.empty((H, W, 3), dtype=torch.float16 if fp16 else torch.float32, device=self.device) if img_out is None else img_out
        if tuple(img.shape) != (H, W, 3) or img.dtype != (torch.float16 if fp16 else torch.float32) or not img.is_contiguous():
            raise ValueError("img_out must be a contiguous [H, W, 3] tensor of the film's type")
        blob = self.blob  # (acquire first: the flag below speaks about the blob this call reads)
        # (the path integrator walks per lane and reads neither apex records nor tile bins: it claims nothing about the blob's apex areas, and rewrites none)
        flags = int(bool(fp16)) | (path if path else self._apex_flag(apex_key(sd)))
        if cache is None:
            mats_arg, lbits, _keep = self._with_lights(sd, albedo, mats_arg, lights, "render_fwd", ambient, lights_directional=lights_directional)
            flags |= lbits
            self._launch_fwd("render_fwd", blob, sd, mats_arg, _dev(tex, name="tex") if tex is not None else None, spp, seed, flags, _dev(img, img.dtype))
            return img
        # ... and the records of the adjoint: one footprint per pixel, under a filtered film every sample's (ABI 7)
        if cache.numel() < render_cache_bytes_sd(sd, spp):
            raise ValueError("cache tensor too small")
        flags |= (_abi.RENDER_SPARSE_ADJOINT if sparse_adjoint else 0) | (_abi.RENDER_CACHE_ZEROED if cache_zeroed else 0) | (_abi.RENDER_CACHE_KEEP_DROPPED if keep_dropped else 0)
        self._launch("render_fwd", "ffx_render_fwd_cache", _TWIN, blob, sd, (mats_arg, _dev(tex, name="tex") if tex is not None else None), spp, seed, flags,
                     _dev(img, img.dtype), _dev(cache, torch.uint8, "cache"))
        return img

    def render_fwd_adjoint(self, sd, albedo, tex, spp, seed, gimg, out=None, dot_out=None, fp16=False, sparse_adjoint=False, img_out=None, max_depth=2):
        """K8 with the adjoint folded in (ffx_render_fwd_adjoint): for a loss whose gradient `gimg` [H,W,3] does not depend on the image.
        -> (img, gtex): the render, and gtex (+)= its adjoint applied to gimg — `out`: accumulate into this [tex_h, tex_w, channels]
        tensor instead of a fresh zeroed one.  dot_out: _abi.ADJOINT_DOT_SLOTS float32 partial sums that <gimg, img> is added to."""
        H, W = sd.cam.height, sd.cam.width
        if sd.rfilter and (dot_out is not None or sd.proj.tex_channels != 1 or sd.n_base_tex > 0):
            raise ValueError("render_fwd_adjoint with a reconstruction filter: 1-channel projector textures, no textured base colours, no dot_out "
                             "(the image forms behind the render launch) — box-filtered pixels are what the general call folds; use render_fwd + render_bwd")
        _no_path(max_depth, "render_fwd_adjoint")
        mats_arg = _check_materials(sd, albedo)
        img = torch.empty((H, W, 3), dtype=torch.float16 if fp16 else torch.float32, device=self.device) if img_out is None else img_out
        if tuple(img.shape) != (H, W, 3) or img.dtype != (torch.float16 if fp16 else torch.float32):
            raise ValueError("img_out must be [H, W, 3] of the film's type")
        gtex = torch.zeros((sd.proj.tex_h, sd.proj.tex_w, sd.proj.tex_channels), dtype=torch.float32, device=self.device) if out is None else out
        if tuple(gimg.shape) != (H, W, 3):
            raise ValueError("gimg must be [H, W, 3]")
        if dot_out is not None and (dot_out.dtype != torch.float32 or dot_out.numel() != _abi.ADJOINT_DOT_SLOTS):
            raise ValueError(f"dot_out must hold {_abi.ADJOINT_DOT_SLOTS} float32 partial sums (the caller zeroes and sums them)")
        blob = self.blob
        flags = int(bool(fp16)) | (_abi.RENDER_SPARSE_ADJOINT if sparse_adjoint else 0) | self._apex_flag(apex_key(sd))
        # (the filtered film — weights -> G, ONE render launch with the adjoint folded in, gather — has its scratch where the box film has dot_out)
        self._launch("render_fwd", "ffx_render_fwd_adjoint", _TWIN, blob, sd, (mats_arg, _dev(tex, name="tex")), spp, seed, flags,
                     _dev(img, img.dtype), _dev(gimg, name="gimg"), _dev(gtex), *(() if sd.rfilter else (_dev(dot_out) if dot_out is not None else None,)))
        return img, gtex

    def render_bwd_cached(self, sd, albedo, cache, spp, gimg, out=None, img=None, dot_out=None, seed=None, max_depth=2):
        """K9 from the adjoint cache written by render_fwd(..., cache=...): scatters per-pixel footprints, no BVH.
        `out`: accumulate into this [tex_h, tex_w, channels] tensor instead of a fresh zeroed one.
        `img` + `dot_out` (render_dot_slots(W, H) float32 partial sums, one per 8x8-pixel block): the same launch adds
        <gimg, img> to them — their sum is the value of a loss that is linear in the image, whose gradient gimg is."""
        _no_path(max_depth, "render_bwd_cached")
        gtex = torch.zeros((sd.proj.tex_h, sd.proj.tex_w, sd.proj.tex_channels), dtype=torch.float32, device=self.device) if out is None else out
        mats_arg = _check_materials(sd, albedo)
        if (img is None) != (dot_out is None):
            raise ValueError("img and dot_out go together")
        if sd.rfilter:  # the filtered film's cache: per-sample records, filter weights re-derived from the forward's seed
            if seed is None or img is not None:
                raise ValueError("render_bwd_cached of a filtered render needs the forward's seed (and has no <gimg, img> output)")
            if tuple(gimg.shape) != (sd.cam.height, sd.cam.width, 3):
                raise ValueError("gimg must be [H, W, 3]")
            with self._timed("render_bwd_cached"):
                self._call("ffx_render_bwd_cached_filtered", C.byref(sd), mats_arg, _dev(cache, torch.uint8, "cache"), int(spp), int(seed) & 0xFFFFFFFF,
                           _dev(gimg, name="gimg"), _dev(gtex), _stream(self._didx))
            return gtex
        if img is not None and (tuple(img.shape) != tuple(gimg.shape) or dot_out.dtype != torch.float32 or dot_out.numel() != render_dot_slots(sd.cam.width, sd.cam.height)):
            raise ValueError("img must have gimg's shape and dot_out must be render_dot_slots(W, H) float32 partial sums (the caller zeroes and sums them)")
        with self._timed("render_bwd_cached"):
            self._call("ffx_render_bwd_cached", C.byref(sd), mats_arg, _dev(cache, torch.uint8, "cache"), int(spp),
                       _dev(gimg, name="gimg"), _dev(gtex), _dev(img, img.dtype, "img") if img is not None else None,
                       int(img is not None and img.dtype == torch.float16), _dev(dot_out) if dot_out is not None else None, _stream(self._didx))
        return gtex

    def render_bwd_cached_l1(self, sd, albedo, cache, spp, img, target, weight, out, loss_slots):
        """K9 under weight * L1Loss(img, target) (ffx_render_bwd_cached_l1): the loss's gradient image is formed inside the scatter launch and the loss value
        goes to `loss_slots` (render_dot_slots(W, H) float32 partial sums) — no loss launch, no gradient image.  -> `out`, or None when the library
        declines the case (FFX_ERR_UNSUPPORTED: the caller takes ffx_l1_value_grad + render_bwd_cached)."""
        if sd.rfilter or img.dtype != torch.float32 or target.dtype != torch.float32 or tuple(img.shape) != (sd.cam.height, sd.cam.width, 3) or tuple(target.shape) != tuple(img.shape):
            return None
        if loss_slots.dtype != torch.float32 or loss_slots.numel() != render_dot_slots(sd.cam.width, sd.cam.height):
            raise ValueError("loss_slots must be render_dot_slots(W, H) float32 partial sums")
        mats_arg = _check_materials(sd, albedo)
        with self._timed("render_bwd_cached"):
            rc = api().call_rc("ffx_render_bwd_cached_l1", C.byref(sd), mats_arg, _dev(cache, torch.uint8, "cache"), int(spp), _dev(img, name="img"), _dev(target, name="target"),
                               float(weight), _dev(out), _dev(loss_slots), _stream(self._didx), allow=(_abi.FFX_ERR_UNSUPPORTED,))
        return out if rc == 0 else None

    def render_bwd_det_part(self, sd, albedo, spp, seed, gimg, part, acc, scale_log2=0, max_depth=2):
        """ONE pass of the deterministic re-tracing adjoint (ffx_render_bwd_det_part): part 1 — the largest |tap| of this render into the int32
        word `acc` (the float's bits; maximum over calls); part 2 — every tap as a 64-bit fixed-point integer at 2^scale_log2 into the int64
        tensor `acc` [tex_h, tex_w, channels] (sum over calls).  The caller clears `acc`, reduces it over samples and ranks, and converts
        (det_scale_log2, det_finish_): sums that come out bitwise equal whatever the order or the number of ranks."""
        _no_path(max_depth, "render_bwd_det_part")
        if _lane_kernels():
            raise ValueError("the per-lane kernels (FFX_TRAVERSAL=lane) have no deterministic adjoint")
        want = torch.int32 if part == 1 else torch.int64
        if acc.dtype != want or not acc.is_contiguous() or (part == 2 and acc.numel() != sd.proj.tex_h * sd.proj.tex_w * sd.proj.tex_channels):
            raise ValueError("render_bwd_det_part: acc must be one int32 word (part 1) / an int64 tensor of the texture's size (part 2)")
        mats_arg = _check_materials(sd, albedo)
        blob = self.blob
        flags = self._apex_flag(apex_key(sd))
        self._launch("render_bwd", "ffx_render_bwd_det_part", _SLOT, blob, sd, (mats_arg,), spp, seed, flags,
                     _dev(gimg, name="gimg"), int(part), int(scale_log2), C.c_void_p(acc.data_ptr()))

    def render_bwd(self, sd, albedo, spp, seed, gimg, deterministic=None, max_depth=2, rr_depth=5, appearance=False, tex=None, material=False, lights=None,
                   ambient=None, lights_directional=False, emitters=False):
        """the re-tracing adjoint.  deterministic (default: FFX_DETERMINISTIC=1 in the environment): ffx_render_bwd_det — bitwise
        reproducible accumulation (64-bit fixed point instead of float atomics; two re-traces and one host synchronisation).
        max_depth > 2: the path integrator's adjoint — replays render_fwd's paths of the same max_depth, rr_depth, spp and seed (float atomics only).
        appearance=True (FFX_RENDER_GRAD_APPEARANCE): -> (gtex, AppearanceGrad) — also d loss / d base colour per material row, d loss /
        d spot intensity and d loss / d base-colour texture; `tex` is the forward's projector texture (needed when the scene has a projector).
        Direct light (max_depth 2) and the float-atomic adjoint only.
        material=True (with appearance=True; FFX_RENDER_GRAD_MATERIAL): AppearanceGrad.material also holds d loss / d the principled BSDF's
        parameters per material row [n_shapes, 11].
        lights: the forward's extra emitters.  They do not depend on the projector's texture: gtex is that of the call without them (the float-atomic
        adjoint is handed the forward's bits and ignores them; the deterministic one is called without).  Not with appearance=True.
        ambient: the forward's constant emitter — as lights: its bit is handed on and ignored.  Not with appearance=True.
        lights_directional: the forward's — handed on with the lights' bits and ignored.
        emitters=True (FFX_RENDER_EMITTER_GRAD): -> (gtex, EmitterGrad) — also d loss / d (the RGB power of every record of `lights`) and
        d loss / d (the radiance of `ambient`): the exact derivative of the fixed-seed image of render_fwd with the same lights, ambient, max_depth,
        rr_depth, spp and seed.  Needs lights= and / or ambient=; the table then travels and is read.  No atomics: two calls give the same EmitterGrad.
        Direct light and max_depth > 2, both films; not with appearance=True, no deterministic adjoint."""
        if ambient is not None and appearance:
            raise NotImplementedError("render_bwd(appearance=True): the constant emitter (ambient=) is not differentiated")
        if lights is not None and lights.numel() and appearance:
            raise NotImplementedError("render_bwd(appearance=True): extra emitters (lights=) are not differentiated")
        if material and not appearance:
            raise ValueError("render_bwd(material=True) needs appearance=True (the material block extends the appearance adjoint)")
        if emitters and appearance:
            raise NotImplementedError("render_bwd(emitters=True): not served together with appearance=True")
        if emitters:
            return self._render_bwd_emitters(sd, albedo, spp, seed, gimg, deterministic, max_depth, rr_depth, lights, ambient, lights_directional)
        if appearance:
            if max_depth != 2:
                path_flags(max_depth)  # (the range check's message first)
                raise ValueError("render_bwd(appearance=True): the appearance gradients are served at max_depth 2 (direct light) only")
            if deterministic is None:
                deterministic = deterministic_mode()
            if deterministic:
                raise ValueError("render_bwd(appearance=True) has no deterministic adjoint (FFX_DETERMINISTIC / deterministic=True)")
            return self._render_bwd_leaves(sd, albedo, spp, seed, gimg, tex, material, 0, "render_bwd(appearance=True)")
        path = path_flags(max_depth, rr_depth) if max_depth != 2 else 0
        if deterministic is None:
            deterministic = deterministic_mode()
        if path and deterministic:
            raise ValueError("render_bwd: max_depth > 2 has no deterministic adjoint (FFX_DETERMINISTIC / deterministic=True)")
        gtex = torch.zeros((sd.proj.tex_h, sd.proj.tex_w, sd.proj.tex_channels), dtype=torch.float32, device=self.device)
        mats_arg = _check_materials(sd, albedo)
        blob = self.blob
        if deterministic:
            if _lane_kernels():
                raise ValueError("the per-lane kernels (FFX_TRAVERSAL=lane) have no deterministic adjoint")
            flags = self._apex_flag(apex_key(sd))
            work = torch.empty(api().lib.ffx_render_bwd_det_bytes(C.byref(sd)), dtype=torch.uint8, device=self.device)  # (a filtered film's scratch is part of it)
            self._launch("render_bwd", "ffx_render_bwd_det", _OWN, blob, sd, (mats_arg,), spp, seed, flags, _dev(gimg, name="gimg"), _dev(gtex), _dev(work, torch.uint8))
            return gtex
        # (the path replay walks per lane: no apex records are read or written.  ABI 7: the direct-light adjoints take FFX_RENDER_APEX_READY like the
        # renders.  Before, they always re-ran the pre-pass — and rewrote the tile bins under the eyes of renders of the same pose on the scene's other
        # render stream)
        flags = path if path else self._apex_flag(apex_key(sd))
        if lights is not None and lights.numel():  # (accepted and ignored: the table's tail is not read, so the table alone travels)
            if lights.dim() != 2 or lights.shape[0] > _abi.RENDER_MAX_LIGHTS:
                raise ValueError(f"render_bwd: lights must be [n <= {_abi.RENDER_MAX_LIGHTS}, {_abi.LIGHT_FLOATS}]")
            flags |= _abi.render_lights(lights.shape[0]) | (_abi.RENDER_LIGHTS_DIRECTIONAL if lights_directional else 0)
        if ambient is not None:  # (accepted and ignored likewise)
            pack_ambient(ambient)
            flags |= _abi.RENDER_AMBIENT
        self._launch_bwd(blob, sd, mats_arg, spp, seed, flags, _dev(gimg, name="gimg"), _dev(gtex))
        return gtex

    def _render_bwd_emitters(self, sd, albedo, spp, seed, gimg, deterministic, max_depth, rr_depth, lights, ambient, lights_directional, out=None):
        """the call behind render_bwd(emitters=True): [table | lights | ambient] travels as in the forward; gtex, the result block and the workspace in one
        buffer (include/ffx.h FFX_RENDER_EMITTER_GRAD).  out: that buffer, the caller's (float32, on the device; its gtex part is zeroed here)"""
        if (lights is None or lights.numel() == 0) and ambient is None:
            raise ValueError("render_bwd(emitters=True) needs lights= and / or ambient=: there is nothing to differentiate")
        path = path_flags(max_depth, rr_depth) if max_depth != 2 else 0
        if deterministic is None:
            deterministic = deterministic_mode()
        if deterministic:
            raise ValueError("render_bwd(emitters=True) has no deterministic adjoint (FFX_DETERMINISTIC / deterministic=True)")
        H, W = sd.cam.height, sd.cam.width
        if gimg.numel() < H * W * 3:
            raise ValueError("gimg must hold [H, W, 3] floats")
        n_tex = sd.proj.tex_h * sd.proj.tex_w * sd.proj.tex_channels
        mats_arg = _check_materials(sd, albedo)
        mats_arg, lbits, _keep = self._with_lights(sd, albedo, mats_arg, lights, "render_bwd(emitters=True)", ambient, lights_directional=lights_directional)
        n = (lbits & _abi.RENDER_LIGHTS_MASK) >> _abi.RENDER_LIGHTS_SHIFT
        # (gtex is accumulated into: zeros; the block and the workspace are written by the call)
        n_out = n_tex + _abi.emitter_grad_floats(W, H)
        if out is None:
            out = torch.empty(n_out, dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or out.dim() != 1 or out.numel() < n_out or not out.is_contiguous():
            raise ValueError(f"render_bwd(emitters=True): out must be a contiguous float32 vector of at least {n_out} floats")
        out[:n_tex].zero_()
        blob = self.blob
        flags = (path if path else self._apex_flag(apex_key(sd))) | lbits | _abi.RENDER_EMITTER_GRAD
        self._launch_bwd(blob, sd, mats_arg, spp, seed, flags, _dev(gimg, name="gimg"), _dev(out))
        block = out[n_tex:n_tex + _abi.RENDER_EMITTER_GRAD_BLOCK_FLOATS].view(_abi.RENDER_MAX_LIGHTS + 1, 3)
        return (out[:n_tex].view(sd.proj.tex_h, sd.proj.tex_w, sd.proj.tex_channels),
                EmitterGrad(block[:n].clone(), block[_abi.RENDER_MAX_LIGHTS].clone() if ambient is not None else None))

    def render_bwd_prb(self, sd, albedo, spp, seed, gimg, tex, max_depth, rr_depth=5, material=False, deterministic=None):
        """path replay backpropagation (Mitsuba's `prb`, FFX_RENDER_GRAD_PRB): -> (gtex, AppearanceGrad) of a render_fwd with the same
        max_depth, rr_depth, spp and seed — render_bwd(appearance=True[, material=True])'s blocks through every bounce, with the texture gradient of
        render_bwd(max_depth=...) from the same launch.  The roulette's decisions and survival probabilities are constants of the replay.  max_depth 2
        is render_bwd(appearance=True).  `tex`: the forward's projector texture (None without a projector).  Float atomics only."""
        path = path_flags(max_depth, rr_depth)
        if deterministic is None:
            deterministic = deterministic_mode()
        if deterministic:
            raise ValueError("render_bwd_prb has no deterministic adjoint (FFX_DETERMINISTIC / deterministic=True)")
        return self._render_bwd_leaves(sd, albedo, spp, seed, gimg, tex, material, (path | _abi.RENDER_GRAD_PRB) if path else 0, "render_bwd_prb")

    def render_jvp(self, sd, albedo, tex, spp, seed=0, *, dtex=None, tangent=None, max_depth=2, rr_depth=5):
        """forward mode (FFX_RENDER_TANGENT): -> (img, dimg), img the image of render_fwd with the same arguments bit for bit and dimg =
        d img / d theta . dtheta.  dtex: the tangent of the projector's texture (shaped like tex); tangent: an AppearanceGrad whose fields hold tangents
        where render_bwd(appearance=True, material=True) returns gradients — rows [n_shapes, 3], spot [3], base_tex [h, w, 3] per texture, material
        [n_shapes, 11] (the eta column: a tangent of eta).  None anywhere is a zero tangent.  albedo: the device material table (needed even when the
        scene description carries the rows).  max_depth > 2: through the bounces with prb's detached roulette.  fp32 film; two calls give the same bits."""
        path = path_flags(max_depth, rr_depth) if max_depth != 2 else 0
        H, W = sd.cam.height, sd.cam.width
        if albedo is None:
            raise ValueError("render_jvp: the device material table is needed")
        _check_table(sd, albedo)
        buf = self.pack_tangent(sd, tex, dtex, tangent).to(self.device)
        out = torch.empty((2, H, W, 3), dtype=torch.float32, device=self.device)
        blob = self.blob
        # (direct light: the primal is the packet kernels' and takes the apex flag render_fwd takes; deeper paths walk per lane)
        flags = (path if path else self._apex_flag(apex_key(sd))) | _abi.RENDER_TANGENT
        self._launch_fwd("render_jvp", blob, sd, _dev(albedo, name="albedo"), _dev(buf, name="tex"), spp, seed, flags, _dev(out))
        return out[0], out[1]

    def render_aov(self, sd, albedo, tex, spp, seed=0, *, max_depth=2, rr_depth=5, lights=None, ambient=None, lights_directional=False):
        """the render and its ground truth (FFX_RENDER_AOV): -> (img [H, W, 3], aov [H, W, 17]), img the image of render_fwd with the
        same arguments bit for bit, aov the primary hit's depth, position, normals, uv, base colour and ids (AOV_CHANNELS names the offsets) through the
        same film over the same samples.  max_depth > 2 chooses the image only.  fp32 film; two calls give the same bits.  lights (pack_lights, as
        render_fwd): the image carries the extra emitters, the block is that of the call without them.  ambient, lights_directional: likewise."""
        path = path_flags(max_depth, rr_depth) if max_depth != 2 else 0
        H, W = sd.cam.height, sd.cam.width
        mats_arg = _check_materials(sd, albedo)
        mats_arg, lbits, _keep = self._with_lights(sd, albedo, mats_arg, lights, "render_aov", ambient, lights_directional=lights_directional)
        out = torch.empty(H * W * (3 + _abi.RENDER_AOV_FLOATS), dtype=torch.float32, device=self.device)
        blob = self.blob
        # (the block's launch reads the camera's apex records and bins: behind a path render, which writes none, the call runs the pre-pass itself unless
        # the blob already holds this pose's)
        flags = path | self._apex_flag(apex_key(sd)) | _abi.RENDER_AOV | lbits
        self._launch_fwd("render_aov", blob, sd, mats_arg, _dev(tex, name="tex") if tex is not None else None, spp, seed, flags, _dev(out))
        return out[:H * W * 3].view(H, W, 3), out[H * W * 3:].view(H, W, _abi.RENDER_AOV_FLOATS)

    @staticmethod
    def pack_tangent(sd, tex, dtex, tangent):
        """the `tex` buffer of a FFX_RENDER_TANGENT call (include/ffx.h): [texture, its tangent] with a projector, then the appearance block's
        _abi.appearance_floats floats of tangent, then — a table with material columns — _abi.material_floats floats.  On the device of `tex` (or of the
        first tangent given, else the host)"""
        S = int(sd.n_shapes)
        bt = [(int(sd.base_tex_h[k]), int(sd.base_tex_w[k])) for k in range(sd.n_base_tex)]
        n_tex = sd.proj.tex_h * sd.proj.tex_w * sd.proj.tex_channels if sd.proj.enabled else 0
        n_mat = _abi.material_floats(S) if int(sd.mat_stride) == _abi.MAT_STRIDE else 0
        t = tangent if tangent is not None else AppearanceGrad(None, None, None, None)
        given = [x for x in (tex, dtex, t.rows, t.spot, t.material, *(t.base_tex or [])) if isinstance(x, torch.Tensor)]
        device = given[0].device if given else torch.device("cpu")
        buf = torch.zeros(2 * n_tex + _abi.appearance_floats(S, bt) + n_mat, dtype=torch.float32, device=device)
        both = buf[:2 * n_tex].view(2, n_tex)
        dst, _ = appearance_blocks(sd, n_mat > 0, buf, 2 * n_tex)

        def put(view, v, what):
            if v is None:
                return
            v = torch.as_tensor(v).detach().to(device=device, dtype=torch.float32).reshape(-1)
            if v.numel() != view.numel():
                raise ValueError(f"render_jvp: {what} must hold {view.numel()} floats, got {v.numel()}")
            view.copy_(v.view(view.shape))

        if n_tex:
            if tex is None:
                raise ValueError(f"render_jvp: the projector's texture ({n_tex} floats) is needed")
            put(both[0], tex, "tex")
            put(both[1], dtex, "dtex")
        put(dst.rows, t.rows, "tangent.rows")
        put(dst.spot, t.spot, "tangent.spot")
        if t.base_tex is not None and len(t.base_tex) != len(bt):
            raise ValueError(f"render_jvp: tangent.base_tex must list {len(bt)} textures (None for a zero tangent)")
        for k, view in enumerate(dst.base_tex):
            put(view, t.base_tex[k] if t.base_tex is not None else None, f"tangent.base_tex[{k}]")
        if t.material is not None and not n_mat:
            raise ValueError("render_jvp: tangent.material on a table without material columns")
        put(dst.material, t.material, "tangent.material")
        return buf

    def _render_bwd_leaves(self, sd, albedo, spp, seed, gimg, tex, material, path, what):
        """the call behind render_bwd(appearance=True) (path 0) and render_bwd_prb (the path bits | FFX_RENDER_GRAD_PRB): gimg and the texture travel in one
        buffer, gtex and the blocks in another (include/ffx.h)"""
        H, W = sd.cam.height, sd.cam.width
        n_tex = sd.proj.tex_h * sd.proj.tex_w * sd.proj.tex_channels
        bt = [(int(sd.base_tex_h[k]), int(sd.base_tex_w[k])) for k in range(sd.n_base_tex)]
        src = gimg.reshape(-1)
        if sd.proj.enabled:
            if tex is None or tex.numel() != n_tex:
                raise ValueError(f"{what}: the forward's projector texture ({n_tex} floats) is needed")
            src = torch.cat([gimg.reshape(-1).float(), tex.detach().reshape(-1).to(device=self.device, dtype=torch.float32)])
        if src.numel() < H * W * 3:
            raise ValueError("gimg must hold [H, W, 3] floats")
        n_mat = _abi.material_floats(sd.n_shapes) if material else 0
        out = torch.zeros(n_tex + _abi.appearance_floats(sd.n_shapes, bt) + n_mat, dtype=torch.float32, device=self.device)
        mats_arg = _check_materials(sd, albedo)
        blob = self.blob
        # (the path replay walks per lane: no apex records are read or written)
        flags = (path if path else self._apex_flag(apex_key(sd))) | _abi.RENDER_GRAD_APPEARANCE | (_abi.RENDER_GRAD_MATERIAL if material else 0)
        self._launch_bwd(blob, sd, mats_arg, spp, seed, flags, _dev(src, name="gimg"), _dev(out))
        return out[:n_tex].view(sd.proj.tex_h, sd.proj.tex_w, sd.proj.tex_channels), appearance_blocks(sd, material, out, n_tex)[0]
