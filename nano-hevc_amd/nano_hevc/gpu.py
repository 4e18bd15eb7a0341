"""Batched, device-resident entry points (the frame-level path).

The reference functions are one block per call; these take whole device
buffers (torch tensors on an MI355X, used only as device memory + stream) and
launch the gfx950 kernels through the C ABI on the tensor's current stream.

  fwd8x8_quant        -- the hot path: fused 8x8 DCT + quant over plane sets
  yuv420_plane_sets   -- nh_plane_set descriptors for a stream of YUV420 frames
  fwd_transform_batch / inv_transform_batch / quant_batch / dequant_batch
  intra_rdo_plane     -- config 3: 35-mode RDO per 8x8 block of a plane; intra_rdo_planes: over plane sets
  intra_rdo_planes_n  -- config 3 at N = 4 (DST / DCT), 8, 16, 32 over plane sets; intra_rdo_plane_n: one plane
  intra_rdo_closed    -- config 3 in closed loop (row wavefront); _yuv420_stream: in batches, several in flight
  dequant_inv8x8      -- decoder stage R: dequantise + inverse 8x8 DCT over plane sets (fwd8x8_quant's mirror)
  intra_decode_closed -- the decoder of intra_rdo_closed: modes + levels -> its reconstruction
  dequant_inv_n       -- decoder stage R at N = 4 (DST / DCT), 8, 16, 32 over plane sets, exact for every level
  intra_decode_closed_n -- the decoder of intra_rdo_closed_n: modes + levels -> its reconstruction
  tu_pipeline_plane   -- config 4: mixed 4..32 TU reconstruction chain on a plane
  tu_pipeline_planes_compact / tu_levels_widen -- config 4 with exact int16 levels (+ int32 spill)
  tc32_plane          -- config 5: 32x32 chain, butterfly or matrix-core variants
  tc32_planes         -- config 5 over a frame stream (one MFMA launch per plane set)
  tc32_planes_compact / tc32_levels_widen -- config 5 with exact int16 / int8 levels (+ int32 spill)
  tu_pipeline_closed  -- config 4 in closed loop (CTU-row wavefront, TUs in z-order)
  tu_pipeline_closed_yuv420 -- the same over a YUV420 stream, luma and chroma wavefronts concurrent
  tu_pipeline_closed_yuv420_stream -- the same in batches of frames, several batches in flight
  tu_pred_map_closed  -- the DC / planar choice per TU of a tu_pipeline_closed call, derived from its outputs
  dequant_inv_tu      -- decoder stage R over a TU map (4x4 DST / DCT, 8, 16, 32), exact for every level
  tu_decode_closed    -- the decoder of tu_pipeline_closed: TU map + pred-mode map + levels -> its reconstruction
  tu_decode_closed_yuv420 -- the same over a YUV420 stream, luma and chroma wavefronts concurrent
  tu_rd_planes        -- config 4 with the quadtree chosen by integer RD cost (open loop); tu_rd_plane, tu_rd_yuv420
  tu_encode_map_planes -- config 4 on a quadtree the caller supplies (open loop)
  widen_u8 / narrow_u8 -- frame I/O casts (YUV420p bytes <-> int16 planes)
  encode_intra_yuv420 -- encode_frame_intra (DC vs planar per block) over a frame stream
  block_server_stop / block_server_set_idle_us / block_server_stats -- the per-block
                        call server: after drop-in per-block calls one
                        workgroup stays resident for its idle time (100 us by default),
                        so a DEVICE-wide synchronize (torch.cuda.synchronize()) right
                        after such calls waits up to that long; block_server_stop()
                        sends it away at once, set_idle_us(0) launches per call instead
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

from . import _lib
from ._lib import PlaneSet, check


def _torch():
    import torch
    return torch


def _stream(stream=None, device=None) -> int:
    """Raw hipStream_t of ``stream``, default: the current stream of ``device``
    (the tensor's device), not of whichever device happens to be current."""
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream(device)
    if device is not None and s.device != device:
        raise ValueError(f"stream on {s.device} but the tensors are on {device}")
    return int(s.cuda_stream)


def _plane_intervals(pset: PlaneSet):
    """[start, end) element range of every plane of a set."""
    span = (pset.height - 1) * pset.pitch + pset.width if pset.height > 0 and pset.width > 0 else 0
    for g in range(pset.num_groups):
        for c in range(pset.planes_per_group):
            b = pset.base + g * pset.group_stride + c * pset.plane_stride
            yield b, b + span


def _set_key(s: PlaneSet):
    return tuple(getattr(s, f) for f, _ in PlaneSet._fields_)


_DISJOINT = {}


def sets_disjoint(a: PlaneSet, b: PlaneSet) -> bool:
    """True when no plane of ``a`` shares an element range with a plane of ``b``
    (memoised: the check walks every plane, ~0.25 ms for 64 frames, and sits before
    the launches of every timed closed-loop call)."""
    key = (_set_key(a), _set_key(b))
    r = _DISJOINT.get(key)
    if r is None:
        if len(_DISJOINT) > 256:
            _DISJOINT.clear()
        r = _DISJOINT[key] = _sets_disjoint(a, b)
    return r


def _sets_disjoint(a: PlaneSet, b: PlaneSet) -> bool:
    iv = sorted([(s, e, 0) for s, e in _plane_intervals(a) if e > s] + [(s, e, 1) for s, e in _plane_intervals(b) if e > s])
    end = {0: -1, 1: -1}
    for s, e, k in iv:
        if s < end[1 - k]:
            return False
        end[k] = max(end[k], e)
    return True


def _need(t, dtype, what):
    torch = _torch()
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{what}: expected a CUDA/HIP torch tensor")
    if t.dtype != dtype:
        raise TypeError(f"{what}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: tensor must be contiguous")


def plane_set(base: int, width: int, height: int, pitch: int | None = None, planes_per_group: int = 1,
              num_groups: int = 1, plane_stride: int = 0, group_stride: int = 0) -> PlaneSet:
    return PlaneSet(base, plane_stride, group_stride, width, height, pitch or width, planes_per_group, num_groups, 0)


def yuv420_frame_elems(width: int, height: int) -> int:
    return width * height + 2 * (width // 2) * (height // 2)


def yuv420_plane_sets(num_frames: int, width: int, height: int, frame_stride: int | None = None,
                      base: int = 0) -> List[PlaneSet]:
    """Descriptors for frames laid out [Y][U][V] back to back (PackedFrame layout):
    one set for the Y planes, one for the U+V planes."""
    fs = frame_stride or yuv420_frame_elems(width, height)
    cw, ch = width // 2, height // 2
    ys = width * height
    return [plane_set(base, width, height, width, 1, num_frames, 0, fs),
            plane_set(base + ys, cw, ch, cw, 2, num_frames, cw * ch, fs)]


def _set_array(sets: Sequence[PlaneSet]):
    """``sets`` as the C array the library takes (an empty list still gets an address)."""
    return (PlaneSet * max(1, len(sets)))(*sets)


def _set_counts(sets: Sequence[PlaneSet], n: int):
    """(full n x n blocks, planes) over every plane of ``sets``."""
    planes = [s.planes_per_group * s.num_groups for s in sets]
    return sum((s.width // n) * (s.height // n) * p for s, p in zip(sets, planes)), sum(planes)


def blocks_in(sets: Sequence[PlaneSet]) -> int:
    return _set_counts(sets, 8)[0]


DEFAULT_VARIANT = 4341   # nontemporal loads+stores, >= 5 waves/SIMD, XCD-aware order (see nh_fused8x8.hip)
PRODUCT_VARIANTS = (DEFAULT_VARIANT, 5)   # 5: the same without the XCD order; the rest are A/B forms (make ab)


def sets_fit(sets: Sequence[PlaneSet], numel: int, what: str):
    """Host-side bounds check before a launch: every plane of every set must lie
    inside a buffer of ``numel`` elements (a kernel never sees the size)."""
    for s in sets:
        if s.num_groups <= 0 or s.width <= 0 or s.height <= 0:
            continue
        last = s.base + (s.num_groups - 1) * s.group_stride + (s.planes_per_group - 1) * s.plane_stride + \
            (s.height - 1) * s.pitch + s.width
        if s.base < 0 or s.plane_stride < 0 or s.group_stride < 0 or last > numel:
            raise ValueError(f"{what}: a plane set reaches outside the buffer ({last} > {numel} elements)")


def sets_fit_rows(sets: Sequence[PlaneSet], numel: int, row_lo: int, row_hi: int, what: str):
    """Like sets_fit, for a launch that touches only rows [row_lo, row_hi) of each
    plane (a band of CTU rows plus the source row above it): those rows must lie
    inside the buffer; the set's base may then point before it (a band-local
    buffer described as rows of the full plane, shard.Cfg4Layout)."""
    for s in sets:
        lo, hi = max(0, row_lo), min(s.height, row_hi)
        if s.num_groups <= 0 or s.width <= 0 or hi <= lo:
            continue
        if s.plane_stride < 0 or s.group_stride < 0:
            raise ValueError(f"{what}: negative plane strides")
        first = s.base + lo * s.pitch
        last = s.base + (s.num_groups - 1) * s.group_stride + (s.planes_per_group - 1) * s.plane_stride + \
            (hi - 1) * s.pitch + s.width
        if first < 0 or last > numel:
            raise ValueError(f"{what}: rows [{lo}, {hi}) of a plane set reach outside the buffer "
                             f"([{first}, {last}) vs {numel} elements)")


def fwd8x8_quant(res, sets: Sequence[PlaneSet], qp: int = 32, is_intra: bool = True, out=None,
                 variant: int = DEFAULT_VARIANT, stream=None):
    """Forward 8x8 DCT (transform.py:154-196) + quantize_block (quant.py:126-137) on
    every full 8x8 block of the int16 planes described by ``sets`` inside ``res``.
    Levels land at the same raster positions of ``out`` (int16)."""
    torch = _torch()
    _need(res, torch.int16, "fwd8x8_quant(res)")
    if out is None:
        out = torch.zeros_like(res)
    _need(out, torch.int16, "fwd8x8_quant(out)")
    sets_fit(sets, min(res.numel(), out.numel()), "fwd8x8_quant")
    arr = _set_array(sets)
    L = _lib.load() if int(variant) in PRODUCT_VARIANTS else _lib.load_ab()   # the A/B forms live in the A/B build
    check(L.nh_fwd8x8_quant_planes_variant(res.data_ptr(), out.data_ptr(), arr, len(sets), int(qp),
                                           int(bool(is_intra)), int(variant), C.c_void_p(_stream(stream, res.device))),
          "fwd8x8_quant", L)
    return out


def fwd8x8_quant_ex(res, sets: Sequence[PlaneSet], qp: int = 32, is_intra: bool = True, out=None,
                    nnz: bool = True, bits: bool = True, stream=None):
    """fwd8x8_quant plus the level-side helpers of quant.py:153-178 per block,
    fused.  Returns (levels, nnz, bits): nnz = count_nonzero
    (uint8; is_all_zero == nnz == 0) and bits = int(estimate_bits) (int32) of
    every full 8x8 block, numbered set by set in the launch's order; either may
    be skipped (None)."""
    torch = _torch()
    _need(res, torch.int16, "fwd8x8_quant_ex(res)")
    if out is None:
        out = torch.zeros_like(res)
    _need(out, torch.int16, "fwd8x8_quant_ex(out)")
    sets_fit(sets, min(res.numel(), out.numel()), "fwd8x8_quant_ex")
    nb = blocks_in(sets)
    t_nnz = torch.empty(nb, dtype=torch.uint8, device=res.device) if nnz else None
    t_bits = torch.empty(nb, dtype=torch.int32, device=res.device) if bits else None
    arr = _set_array(sets)
    check(_lib.load().nh_fwd8x8_quant_planes_ex(
        res.data_ptr(), out.data_ptr(), arr, len(sets), int(qp), int(bool(is_intra)),
        t_nnz.data_ptr() if nnz else None, t_bits.data_ptr() if bits else None, C.c_void_p(_stream(stream, res.device))))
    return out, t_nnz, t_bits


def fwd8x8_quant_plane(res2d, qp: int = 32, is_intra: bool = True, out=None, stream=None):
    """One raster int16 plane (H, W); W must be a multiple of 8 (row pitch = W)."""
    h, w = res2d.shape
    return fwd8x8_quant(res2d, [plane_set(0, w, h, w)], qp, is_intra, out, stream=stream)


def _blocks(x, what):
    torch = _torch()
    _need(x, torch.int32, what)
    if x.dim() != 3 or x.shape[1] != x.shape[2]:
        raise ValueError(f"{what}: expected (B, N, N) int32")
    return x.shape[0], x.shape[1]


def fwd_transform_batch(x, use_dst: bool = False, out=None, stream=None):
    """(B, N, N) int32 -> forward_transform of every block (transform.py:154-196)."""
    b, n = _blocks(x, "fwd_transform_batch")
    out = _torch().empty_like(x) if out is None else out
    check(_lib.load().nh_fwd_transform_batch(x.data_ptr(), out.data_ptr(), b, n, int(bool(use_dst)),
                                             C.c_void_p(_stream(stream, x.device))), "fwd_transform_batch")
    return out


def inv_transform_batch(x, use_dst: bool = False, out=None, stream=None):
    """(B, N, N) int32 -> inverse_transform of every block (transform.py:199-238)."""
    b, n = _blocks(x, "inv_transform_batch")
    out = _torch().empty_like(x) if out is None else out
    check(_lib.load().nh_inv_transform_batch(x.data_ptr(), out.data_ptr(), b, n, int(bool(use_dst)),
                                             C.c_void_p(_stream(stream, x.device))), "inv_transform_batch")
    return out


def quant_batch(c, qp: int, log2size: int, is_intra: bool = True, out=None, stream=None):
    """Elementwise quantize (quant.py:41-79) of an int32 tensor."""
    torch = _torch()
    _need(c, torch.int32, "quant_batch")
    out = torch.empty_like(c) if out is None else out
    check(_lib.load().nh_quant_batch(c.data_ptr(), out.data_ptr(), c.numel(), int(qp), int(log2size),
                                     int(bool(is_intra)), C.c_void_p(_stream(stream, c.device))), "quant_batch")
    return out


def dequant_batch(l, qp: int, out=None, stream=None):
    """Elementwise dequantize (quant.py:82-123) of an int32 tensor."""
    torch = _torch()
    _need(l, torch.int32, "dequant_batch")
    out = torch.empty_like(l) if out is None else out
    check(_lib.load().nh_dequant_batch(l.data_ptr(), out.data_ptr(), l.numel(), int(qp),
                                       C.c_void_p(_stream(stream, l.device))), "dequant_batch")
    return out


def intra_rdo_plane(src, qp: int = 32, pitch: int | None = None, stream=None):
    """Config 3 on one int16 plane (H, W): returns
    (modes u8 (H/8, W/8), levels int32 (H, W), recon int16 (H, W), sse int64 (1,))."""
    torch = _torch()
    _need(src, torch.int16, "intra_rdo_plane")
    h, w = src.shape
    dev = src.device
    modes = torch.zeros((h // 8, w // 8), dtype=torch.uint8, device=dev)
    lvl = torch.zeros((h, w), dtype=torch.int32, device=dev)
    rec = torch.zeros((h, w), dtype=torch.int16, device=dev)
    sse = torch.zeros(1, dtype=torch.int64, device=dev)
    check(_lib.load().nh_intra_rdo_plane(src.data_ptr(), w, h, pitch or w, int(qp), modes.data_ptr(), lvl.data_ptr(),
                                         rec.data_ptr(), sse.data_ptr(), C.c_void_p(_stream(stream, src.device))), "intra_rdo_plane")
    return modes, lvl, rec, sse


def _rdo_prepare(what: str, src, sets: Sequence[PlaneSet], block_size: int, lvl, rec, stats: bool = False):
    """Argument checks and default outputs of the config-3 encoders; returns (n, lvl, rec,
    modes, acc, nmodes, nplanes).  ``acc`` holds the per-plane sums: sse int64 (planes,),
    zeroed for the kernels to add to, or with ``stats`` (the RD forms, DESIGN.md §3.3b,
    §3.7b) int64 (planes, 3), overwritten by the call."""
    torch = _torch()
    _need(src, torch.int16, f"{what}(src)")
    n = int(block_size)
    if n not in (4, 8, 16, 32):
        raise ValueError(f"{what}: block_size must be 4, 8, 16 or 32, got {block_size}")
    sets_fit(sets, src.numel(), what)
    nmodes, nplanes = _set_counts(sets, n)
    dev = src.device
    if lvl is None:
        lvl = torch.zeros(src.shape, dtype=torch.int32, device=dev)
    if rec is None:
        rec = torch.zeros(src.shape, dtype=torch.int16, device=dev)
    _need(lvl, torch.int32, f"{what}(lvl)")
    _need(rec, torch.int16, f"{what}(rec)")
    if lvl.numel() < src.numel() or rec.numel() < src.numel():
        raise ValueError(f"{what}: lvl / rec smaller than src")
    modes = torch.zeros(max(1, nmodes), dtype=torch.uint8, device=dev)
    if stats:
        acc = torch.empty((max(1, nplanes), 3), dtype=torch.int64, device=dev)
    else:
        acc = torch.zeros(max(1, nplanes), dtype=torch.int64, device=dev)
    return n, lvl, rec, modes, acc, nmodes, nplanes


def _rdo_rd_prepare(what: str, src, sets: Sequence[PlaneSet], block_size: int, lam: int, lvl, rec):
    if not 0 <= int(lam) <= 2 ** 31 - 1:
        raise ValueError(f"{what}: lam (lambda) must be in 0..2^31-1")
    return _rdo_prepare(what, src, sets, block_size, lvl, rec, stats=True)


def _closed_status(work, st: int, what: str, status2: str | None = None):
    """Read the status word of a closed-loop call's workspace on stream ``st`` (a host round
    trip): 0 returns; 2 raises ValueError with ``status2`` where the call has such a
    refusal (a bad map); anything else is a stalled wavefront, RuntimeError."""
    status = C.c_int(0)
    check(_lib.load().nh_intra_rdo_closed_status(work.data_ptr(), C.byref(status), C.c_void_p(st)))
    if status.value == 2 and status2:
        raise ValueError(f"{what}: {status2}")
    if status.value:
        raise RuntimeError("%s: the device wavefront stalled (status %d)" % (what, status.value))


def _closed_call(what: str, wb: int, dev, stream, call, status2: str | None = None):
    """The end of a closed-loop config-3 call.  ``wb``: the library's workspace size for
    it, negative for a refusal (ValueError with the library's text); ``call(work, st)``
    makes the library call on a fresh workspace; then the status word is checked."""
    if wb < 0:
        raise ValueError(f"{what}: bad plane sets or argument: " + _lib.load().nh_last_error().decode(errors="replace"))
    work = _torch().empty(max(2, (wb + 7) // 8 * 2), dtype=_torch().int32, device=dev)
    st = _stream(stream, dev)
    check(call(work.data_ptr(), C.c_void_p(st)), what)
    _closed_status(work, st, what, status2)


def intra_rdo_planes(src, sets: Sequence[PlaneSet], qp: int = 32, lvl=None, rec=None, stream=None):
    """Config 3 over every plane of ``sets`` -- a frame stream
    in one launch pair per set instead of a launch per plane.  Returns (modes
    uint8 [sum of per-plane (h/8)*(w/8), set order], lvl int32, recon int16
    (source layout), sse int64 per plane); the same results as ``intra_rdo_plane``
    plane by plane."""
    what = "intra_rdo_planes"
    _, lvl, rec, modes, sse, nmodes, nplanes = _rdo_prepare(what, src, sets, 8, lvl, rec)
    check(_lib.load().nh_intra_rdo_planes(src.data_ptr(), _set_array(sets), len(sets), int(qp), modes.data_ptr(),
                                          lvl.data_ptr(), rec.data_ptr(), sse.data_ptr(),
                                          C.c_void_p(_stream(stream, src.device))), what)
    return modes[:nmodes], lvl, rec, sse[:nplanes]


def intra_rdo_planes_n(src, sets: Sequence[PlaneSet], block_size: int, qp: int = 32, use_dst: bool = False,
                       lvl=None, rec=None, stream=None):
    """Config 3 at block size N = ``block_size`` in {4, 8, 16, 32}
    over every plane of ``sets``: the best of the 35 intra modes per full NxN
    block, open loop.  ``use_dst`` (N = 4 only) selects the 4x4 DST-VII.  Returns
    (modes uint8 [sum of per-plane (h/N)*(w/N), set order], lvl int32, recon int16
    (source layout; samples outside full blocks keep the caller's contents), sse
    int64 per plane).  A QP outside 0..51 raises ValueError (it is not clamped);
    N = 8 runs the ``intra_rdo_planes`` kernels."""
    what = "intra_rdo_planes_n"
    n, lvl, rec, modes, sse, nmodes, nplanes = _rdo_prepare(what, src, sets, block_size, lvl, rec)
    check(_lib.load().nh_intra_rdo_planes_n(src.data_ptr(), _set_array(sets), len(sets), n, int(bool(use_dst)), int(qp),
                                            modes.data_ptr(), lvl.data_ptr(), rec.data_ptr(), sse.data_ptr(),
                                            C.c_void_p(_stream(stream, src.device))), what)
    return modes[:nmodes], lvl, rec, sse[:nplanes]


def _rdo_one_plane(what: str, planes_fn, src, block_size: int, pitch, *args, stream=None):
    """``planes_fn(buffer, sets, block_size, *args)`` -- ``intra_rdo_planes_n`` or its RD
    form -- on one int16 plane (H, W) whose rows are ``pitch`` (default W) samples apart."""
    torch = _torch()
    _need(src, torch.int16, what)
    h, w = src.shape
    p = int(pitch or w)
    if p < w:
        raise ValueError(f"{what}: pitch < width")
    buf = src
    if p != w:   # rows of the (H, W) tensor re-spaced: run on a pitched copy, return (H, W) views
        buf = torch.zeros((h, p), dtype=torch.int16, device=src.device)
        buf[:, :w] = src
    modes, lvl, rec, acc = planes_fn(buf, [plane_set(0, w, h, p)], block_size, *args, stream=stream)
    if p != w:
        lvl, rec = lvl[:, :w], rec[:, :w]
    n = int(block_size)
    return modes.reshape(h // n, w // n), lvl, rec, acc


def intra_rdo_plane_n(src, block_size: int, qp: int = 32, use_dst: bool = False, pitch: int | None = None,
                      stream=None):
    """``intra_rdo_planes_n`` on one int16 plane (H, W) whose rows are ``pitch`` (default
    W) samples apart: (modes u8 (H/N, W/N), levels int32 (H, W), recon int16 (H, W),
    sse int64 (1,))."""
    return _rdo_one_plane("intra_rdo_plane_n", intra_rdo_planes_n, src, block_size, pitch, qp, use_dst, stream=stream)


def intra_rdo_closed(src, sets: Sequence[PlaneSet], qp: int = 32, lvl=None, rec=None, stream=None):
    """Config 3 in CLOSED loop over every plane of ``sets``:
    raster block order, neighbours from the reconstruction, wavefront schedule
    on the device.  Returns (modes uint8 [sum of per-plane (h/8)*(w/8)],
    lvl int32, recon int16 (source layout), sse int64 per plane).
    Speed note: the packed 16-bit form runs only when EVERY source sample of
    the call (all sets) is in [0, 255]; one sample outside sends the whole call
    to the 32-bit form (same results, ~1.4x the time).  Split
    such streams into separate calls to keep the 8-bit ones fast."""
    what = "intra_rdo_closed"
    _, lvl, rec, modes, sse, nmodes, nplanes = _rdo_prepare(what, src, sets, 8, lvl, rec)
    L = _lib.load()
    arr = _set_array(sets)
    _closed_call(what, int(L.nh_intra_rdo_closed_workspace_bytes(arr, len(sets))), src.device, stream,
                 lambda work, st: L.nh_intra_rdo_planes_closed(src.data_ptr(), arr, len(sets), int(qp), modes.data_ptr(),
                                                               lvl.data_ptr(), rec.data_ptr(), sse.data_ptr(), work, st))
    return modes[:nmodes], lvl, rec, sse[:nplanes]


def intra_rdo_closed_n(src, sets: Sequence[PlaneSet], block_size: int, qp: int = 32, use_dst: bool = False,
                       lvl=None, rec=None, stream=None):
    """Config 3 in CLOSED loop at block size N = ``block_size`` in {4, 8, 16, 32}
     over every plane of ``sets``: the best of the 35 intra modes
    per full NxN block, blocks in raster order, neighbours from the reconstruction,
    row wavefront on the device.  ``use_dst`` (N = 4 only) selects the 4x4 DST-VII.
    Returns (modes uint8 [sum of per-plane (h/N)*(w/N), set order], lvl int32
    (samples outside full blocks keep the caller's contents), recon int16 (0
    outside full blocks), sse int64 per plane).  A bad block size, QP outside
    0..51 or ``use_dst`` with N != 4 raises ValueError; a stalled wavefront raises
    RuntimeError.  N = 8 runs the ``intra_rdo_closed`` kernels."""
    what = "intra_rdo_closed_n"
    n, lvl, rec, modes, sse, nmodes, nplanes = _rdo_prepare(what, src, sets, block_size, lvl, rec)
    L = _lib.load()
    arr = _set_array(sets)
    _closed_call(what, int(L.nh_intra_rdo_closed_n_workspace_bytes(arr, len(sets), n)), src.device, stream,
                 lambda work, st: L.nh_intra_rdo_planes_closed_n(src.data_ptr(), arr, len(sets), n, int(bool(use_dst)),
                                                                 int(qp), modes.data_ptr(), lvl.data_ptr(),
                                                                 rec.data_ptr(), sse.data_ptr(), work, st))
    return modes[:nmodes], lvl, rec, sse[:nplanes]


def intra_rdo_rd_planes_n(src, sets: Sequence[PlaneSet], block_size: int, qp: int = 32, lam: int = 0,
                          use_dst: bool = False, lvl=None, rec=None, stream=None):
    """Config 3 with a rate term, open loop, at block size N =
    ``block_size`` in {4, 8, 16, 32} over every plane of ``sets``: the 35 chains of
    ``intra_rdo_planes_n`` per full NxN block, the winner by J = D + lam * R with
    D = sum (int16)(orig - rec)^2 and R = count_nonzero(level) + 1 (the rate of
    ``tu_rd_planes``), ties to the lowest mode.  ``lam`` 0..2^31-1; ``lam`` = 0 gives
    ``intra_rdo_planes_n``'s modes, levels and recon.  Returns (modes uint8 [sum of
    per-plane (h/N)*(w/N), set order], lvl int32, recon int16 (source layout;
    samples outside full blocks keep the caller's contents), stats int64
    (planes, 3): sum J, sum D, sum R over the plane's blocks, overwritten).  Bad
    arguments raise ValueError (a QP outside 0..51 is not clamped).  N = 8 runs the
    N-lane chains, not the packed ``intra_rdo_planes`` kernels."""
    what = "intra_rdo_rd_planes_n"
    n, lvl, rec, modes, stats, nmodes, nplanes = _rdo_rd_prepare(what, src, sets, block_size, lam, lvl, rec)
    check(_lib.load().nh_intra_rdo_rd_planes_n(src.data_ptr(), _set_array(sets), len(sets), n, int(bool(use_dst)),
                                               int(qp), int(lam), modes.data_ptr(), lvl.data_ptr(), rec.data_ptr(),
                                               stats.data_ptr(), C.c_void_p(_stream(stream, src.device))), what)
    return modes[:nmodes], lvl, rec, stats[:nplanes]


def intra_rdo_rd_plane_n(src2d, block_size: int, qp: int = 32, lam: int = 0, use_dst: bool = False,
                         pitch: int | None = None, stream=None):
    """``intra_rdo_rd_planes_n`` on one int16 plane (H, W) whose rows are ``pitch``
    (default W) samples apart: (modes u8 (H/N, W/N), levels int32 (H, W), recon int16
    (H, W), stats int64 (1, 3))."""
    return _rdo_one_plane("intra_rdo_rd_plane_n", intra_rdo_rd_planes_n, src2d, block_size, pitch, qp, lam, use_dst,
                          stream=stream)


def intra_rdo_rd_closed_n(src, sets: Sequence[PlaneSet], block_size: int, qp: int = 32, lam: int = 0,
                          use_dst: bool = False, lvl=None, rec=None, stream=None):
    """Config 3 with a rate term in CLOSED loop: ``intra_rdo_closed_n``
    with the winner of every block chosen by J = D + lam * R (as
    ``intra_rdo_rd_planes_n``); the neighbours of later blocks come from the J
    winner's reconstruction, and ``intra_decode_closed_n(modes, lvl, ...)`` returns
    ``rec``.  ``lam`` = 0 gives ``intra_rdo_closed_n``'s modes, levels and recon.
    Returns (modes, lvl int32 (samples outside full blocks keep the caller's
    contents), recon int16 (0 outside full blocks), stats int64 (planes, 3): sum J,
    sum D, sum R, overwritten).  Bad arguments raise ValueError; a stalled wavefront
    raises RuntimeError."""
    what = "intra_rdo_rd_closed_n"
    n, lvl, rec, modes, stats, nmodes, nplanes = _rdo_rd_prepare(what, src, sets, block_size, lam, lvl, rec)
    L = _lib.load()
    arr = _set_array(sets)
    _closed_call(what, int(L.nh_intra_rdo_rd_closed_n_workspace_bytes(arr, len(sets), n)), src.device, stream,
                 lambda work, st: L.nh_intra_rdo_rd_planes_closed_n(src.data_ptr(), arr, len(sets), n,
                                                                    int(bool(use_dst)), int(qp), int(lam),
                                                                    modes.data_ptr(), lvl.data_ptr(), rec.data_ptr(),
                                                                    stats.data_ptr(), work, st))
    return modes[:nmodes], lvl, rec, stats[:nplanes]


def _dequant_need(what: str, lvl, out):
    """The checks of a stage-R call's level tensor (int16 or int32) and of its int16 ``out``,
    zero-filled in ``lvl``'s shape by default; returns ``out``."""
    torch = _torch()
    if not isinstance(lvl, torch.Tensor) or lvl.dtype not in (torch.int16, torch.int32):
        raise TypeError(f"{what}(lvl): expected an int16 or int32 CUDA/HIP torch tensor")
    _need(lvl, lvl.dtype, f"{what}(lvl)")
    if out is None:
        out = torch.zeros(lvl.shape, dtype=torch.int16, device=lvl.device)
    _need(out, torch.int16, f"{what}(out)")
    if out.device != lvl.device:
        raise ValueError(f"{what}: out and lvl on different devices")
    return out


def dequant_inv8x8(lvl, sets: Sequence[PlaneSet], qp: int = 32, out=None, stream=None):
    """Stage R of the decoder, the mirror of ``fwd8x8_quant``:
    inverse_transform(dequantize_block(level, qp)).astype(int16) on every full
    8x8 block of the int16 or int32 level planes described by ``sets`` inside
    ``lvl``; exact for every level value of the dtype.  The residual lands at the
    same raster positions of ``out`` (int16, same shape); samples outside full
    blocks are left as they are.  Any pitch >= width and any base."""
    out = _dequant_need("dequant_inv8x8", lvl, out)
    sets_fit(sets, min(lvl.numel(), out.numel()), "dequant_inv8x8")
    check(_lib.load().nh_dequant_inv8x8_planes(lvl.data_ptr(), lvl.element_size(), out.data_ptr(), _set_array(sets),
                                               len(sets), int(qp), C.c_void_p(_stream(stream, lvl.device))),
          "dequant_inv8x8")
    return out


def _decode_closed(what: str, modes, lvl, sets: Sequence[PlaneSet], block_size: int, use_dst, qp: int, rec, stream):
    """``intra_decode_closed_n``; ``use_dst`` None: ``intra_decode_closed``, on the 8x8 entry points."""
    torch = _torch()
    _need(lvl, torch.int32, f"{what}(lvl)")
    _need(modes, torch.uint8, f"{what}(modes)")
    if modes.device != lvl.device:
        raise ValueError(f"{what}: modes and lvl on different devices")
    n = int(block_size)
    if n not in (4, 8, 16, 32):
        raise ValueError(f"{what}: block_size must be 4, 8, 16 or 32, got {block_size}")
    sets_fit(sets, lvl.numel(), what)
    nmodes = _set_counts(sets, n)[0]
    if modes.numel() < nmodes:
        raise ValueError(f"{what}: {modes.numel()} modes for {nmodes} blocks")
    if rec is None:
        rec = torch.zeros(lvl.shape, dtype=torch.int16, device=lvl.device)
    _need(rec, torch.int16, f"{what}(rec)")
    if rec.device != lvl.device:
        raise ValueError(f"{what}: rec and lvl on different devices")
    if rec.numel() < lvl.numel():
        raise ValueError(f"{what}: rec smaller than lvl")
    if nmodes == 0:   # no full block anywhere: the device still zeroes rec, but reads no mode
        modes = torch.zeros(1, dtype=torch.uint8, device=lvl.device)
    L = _lib.load()
    arr = _set_array(sets)
    if use_dst is None:
        wb, entry, form = L.nh_intra_decode_closed_workspace_bytes(arr, len(sets)), L.nh_intra_decode_planes_closed, ()
    else:
        wb, entry = L.nh_intra_decode_closed_n_workspace_bytes(arr, len(sets), n), L.nh_intra_decode_planes_closed_n
        form = (n, int(bool(use_dst)))
    _closed_call(what, int(wb), lvl.device, stream,
                 lambda work, st: entry(modes.data_ptr(), lvl.data_ptr(), arr, len(sets), *form, int(qp), rec.data_ptr(),
                                        work, st), "a mode above 34 in the mode map")
    return rec


def intra_decode_closed(modes, lvl, sets: Sequence[PlaneSet], qp: int = 32, rec=None, stream=None):
    """The decoder of ``intra_rdo_closed``: from that call's
    ``modes`` (uint8, its layout), ``lvl`` (int32, source layout), ``sets`` and
    ``qp``, rebuild its reconstruction -- stage R, then one prediction per block
    in closed loop on the row wavefront.  Returns recon int16 (source layout, 0
    outside full blocks).  A mode above 34 raises ValueError."""
    return _decode_closed("intra_decode_closed", modes, lvl, sets, 8, None, qp, rec, stream)


def dequant_inv_n(lvl, sets: Sequence[PlaneSet], block_size: int, qp: int = 32, use_dst: bool = False, out=None,
                  stream=None):
    """Stage R of the decoder at block size N = ``block_size`` in {4, 8, 16, 32}
    (DESIGN.md §3.9a): inverse_transform(dequantize_block(level, qp), use_dst)
    .astype(int16) on every full NxN block of the int16 or int32 level planes
    described by ``sets`` inside ``lvl``; exact for every level value of the dtype.
    ``use_dst`` (N = 4 only) selects the 4x4 DST-VII.  The residual lands at the
    same raster positions of ``out`` (int16, same shape); samples outside full
    blocks are left as they are.  Any pitch >= width and any base.  A refusal of
    the library (bad block size, ``use_dst`` with N != 4, bad plane sets) raises
    ValueError with its text."""
    out = _dequant_need("dequant_inv_n", lvl, out)
    sets_fit(sets, min(lvl.numel(), out.numel()), "dequant_inv_n")
    check(_lib.load().nh_dequant_inv_planes_n(lvl.data_ptr(), lvl.element_size(), out.data_ptr(), _set_array(sets),
                                              len(sets), int(block_size), int(bool(use_dst)), int(qp),
                                              C.c_void_p(_stream(stream, lvl.device))), "dequant_inv_n")
    return out


def intra_decode_closed_n(modes, lvl, sets: Sequence[PlaneSet], block_size: int, qp: int = 32, use_dst: bool = False,
                          rec=None, stream=None):
    """The decoder of ``intra_rdo_closed_n``: from that call's
    ``modes`` (uint8, its layout), ``lvl`` (int32, source layout), ``sets``,
    ``block_size``, ``use_dst`` and ``qp``, rebuild its reconstruction -- stage R,
    then one prediction per block in closed loop on the row wavefront.  Returns
    recon int16 (source layout, 0 outside full blocks).  QP is clamped to 0..51.
    A mode above 34, too few modes for the blocks or a refusal of the library (bad
    block size, ``use_dst`` with N != 4, bad plane sets) raises ValueError; a
    stalled wavefront raises RuntimeError.  N = 8 runs ``intra_decode_closed``'s
    kernels."""
    return _decode_closed("intra_decode_closed_n", modes, lvl, sets, block_size, bool(use_dst), qp, rec, stream)


def intra_rdo_closed_yuv420_stream(src, width: int, height: int, num_frames: int, qp: int = 32,
                                   batch_frames: int = 64, depth: int = 3, lvl=None, rec=None, stream=None,
                                   frame_stride: int | None = None, base: int = 0):
    """``intra_rdo_closed`` over a stream of YUV420 frames laid out back to back
    (``yuv420_plane_sets``), in batches of ``batch_frames`` frames whose launches
    rotate over ``depth`` streams with no host round trip between them, so a
    batch's block rows fill what the previous batch's wavefront leaves idle while
    it ramps down (1080p: 0.214 vs 0.233 ms per frame for one
    64-frame call).  Same outputs, in the same layout, as one ``intra_rdo_closed``
    call over ``yuv420_plane_sets(num_frames, ...)``: modes and sse of the Y
    planes, then of the U, V planes; lvl / rec in the source layout."""
    torch = _torch()
    if batch_frames < 1 or depth < 1 or num_frames < 0:
        raise ValueError("intra_rdo_closed_yuv420_stream: batch_frames, depth >= 1 and num_frames >= 0")
    fs = frame_stride or yuv420_frame_elems(width, height)
    if fs < yuv420_frame_elems(width, height):
        raise ValueError("intra_rdo_closed_yuv420_stream: frame_stride shorter than a frame")
    all_sets = yuv420_plane_sets(num_frames, width, height, fs, base)
    sets_fit(all_sets, src.numel(), "intra_rdo_closed_yuv420_stream")
    _need(src, torch.int16, "intra_rdo_closed_yuv420_stream(src)")
    dev = src.device
    main = stream if stream is not None else torch.cuda.current_stream(dev)
    if main.device != dev:
        raise ValueError(f"intra_rdo_closed_yuv420_stream: stream on {main.device} but src on {dev}")
    ny = (width // 8) * (height // 8)          # modes per Y plane
    nc = (width // 16) * (height // 16)        # per U / V plane
    with torch.cuda.device(dev), torch.cuda.stream(main):
        if lvl is None:
            lvl = torch.zeros(src.shape, dtype=torch.int32, device=dev)
        if rec is None:
            rec = torch.zeros(src.shape, dtype=torch.int16, device=dev)
        modes = torch.zeros(max(1, num_frames * (ny + 2 * nc)), dtype=torch.uint8, device=dev)
        sse = torch.zeros(max(1, 3 * num_frames), dtype=torch.int64, device=dev)
    _need(lvl, torch.int32, "intra_rdo_closed_yuv420_stream(lvl)")
    _need(rec, torch.int16, "intra_rdo_closed_yuv420_stream(rec)")
    if lvl.numel() < src.numel() or rec.numel() < src.numel():
        raise ValueError("intra_rdo_closed_yuv420_stream: lvl / rec smaller than src")
    if num_frames == 0:
        return modes[:0], lvl, rec, sse[:0]
    L = _lib.load()
    pool = _PIPE_STREAMS3.setdefault(dev.index, [])
    while len(pool) < depth:
        pool.append(torch.cuda.Stream(device=dev))
    fork = torch.cuda.Event()
    fork.record(main)
    for s_ in pool[:depth]:
        s_.wait_event(fork)
    works, keep = [], []
    for b, f0 in enumerate(range(0, num_frames, batch_frames)):
        nb = min(batch_frames, num_frames - f0)
        sets = yuv420_plane_sets(nb, width, height, fs, base + f0 * fs)
        arr = (PlaneSet * 2)(*sets)
        wb = int(L.nh_intra_rdo_closed_workspace_bytes(arr, 2))
        if wb < 0:
            raise ValueError("intra_rdo_closed_yuv420_stream: bad frame size")
        s_ = pool[b % depth]
        with torch.cuda.stream(s_):
            md = torch.empty(nb * (ny + 2 * nc), dtype=torch.uint8, device=dev)
            ss = torch.zeros(3 * nb, dtype=torch.int64, device=dev)   # the kernels add into it
            w_ = torch.empty((wb + 3) // 4, dtype=torch.int32, device=dev)
            check(L.nh_intra_rdo_planes_closed(src.data_ptr(), arr, 2, int(qp), md.data_ptr(), lvl.data_ptr(),
                                               rec.data_ptr(), ss.data_ptr(), w_.data_ptr(), C.c_void_p(s_.cuda_stream)))
            # the batch's modes / sse into the whole stream's layout (Y planes, then U, V planes)
            modes[f0 * ny:(f0 + nb) * ny].copy_(md[:nb * ny])
            modes[num_frames * ny + 2 * f0 * nc:num_frames * ny + 2 * (f0 + nb) * nc].copy_(md[nb * ny:])
            sse[f0:f0 + nb].copy_(ss[:nb])
            sse[num_frames + 2 * f0:num_frames + 2 * (f0 + nb)].copy_(ss[nb:])
        works.append(w_)
        keep += [md, ss]
    for s_ in pool[:depth]:
        join = torch.cuda.Event()
        join.record(s_)
        main.wait_event(join)
    for t in works + keep:
        t.record_stream(main)
    with torch.cuda.device(dev), torch.cuda.stream(main):   # every status word ORed: one host round trip
        both = works[0][:2].clone()
        for w_ in works[1:]:
            both.bitwise_or_(w_[:2])
    _closed_status(both, int(main.cuda_stream), "intra_rdo_closed_yuv420_stream")
    return modes[:num_frames * (ny + 2 * nc)], lvl, rec, sse[:3 * num_frames]


_PIPE_STREAMS3 = {}


def tu_pipeline_plane(src, ctb: int, plane_id: int, seed: int, qp: int = 32, is_luma: bool = True,
                      row0: int = 0, row1: int = 1 << 30, lvl=None, rec=None, tu=None, work=None, stream=None):
    """Config 4 on one int16 plane (H, W), CTU rows [row0, row1).
    Returns (levels int32 (H, W), recon int16 (H, W), tu_log2 u8 (H/4, W/4))."""
    torch = _torch()
    _need(src, torch.int16, "tu_pipeline_plane")
    h, w = src.shape
    dev = src.device
    L = _lib.load()
    lvl = torch.zeros((h, w), dtype=torch.int32, device=dev) if lvl is None else lvl
    rec = torch.zeros((h, w), dtype=torch.int16, device=dev) if rec is None else rec
    tu = torch.zeros((h // 4, w // 4), dtype=torch.uint8, device=dev) if tu is None else tu
    nwork = int(L.nh_tu_workspace_bytes(w, h, ctb))
    if work is None and nwork > 0:
        work = torch.empty(nwork, dtype=torch.uint8, device=dev)
    check(L.nh_tu_pipeline_plane(src.data_ptr(), w, h, w, int(ctb), int(plane_id), int(seed) & 0xFFFFFFFF, int(qp),
                                 int(bool(is_luma)), int(row0), int(min(row1, 1 << 30)), lvl.data_ptr(), rec.data_ptr(),
                                 tu.data_ptr(), work.data_ptr() if work is not None else None,
                                 C.c_void_p(_stream(stream, src.device))), "tu_pipeline_plane")
    return lvl, rec, tu


def tu_pipeline_planes(src, pset: PlaneSet, ctb: int, plane_id: int, seed: int, qp: int = 32, is_luma: bool = True,
                       row0: int = 0, row1: int = 1 << 30, lvl=None, rec=None, tu=None, stream=None):
    """Config 4 over every plane of one plane set in one launch (plane p =
    g*ppg + c gets plane id plane_id + c), CTU rows [row0, row1).  ``lvl`` and
    ``rec`` share the source's layout; the set may describe a band-local buffer
    as rows of the full plane (shard.Cfg4Layout: only the band's rows and the
    row above are read).  Returns (lvl int32, recon int16, tu uint8 (planes,
    h/4, w/4), indexed by full-plane position))."""
    torch = _torch()
    _need(src, torch.int16, "tu_pipeline_planes(src)")
    # the launch reads rows [row0*ctb - 1, row1*ctb) (its CTU rows + the source row above) and writes its CTU rows
    sets_fit_rows([pset], src.numel(), int(row0) * ctb - 1, min(int(row1), 1 << 30) * ctb, "tu_pipeline_planes")
    planes = pset.planes_per_group * pset.num_groups
    if lvl is None:
        lvl = torch.zeros(src.shape, dtype=torch.int32, device=src.device)
    if rec is None:
        rec = torch.zeros(src.shape, dtype=torch.int16, device=src.device)
    if tu is None:
        tu = torch.zeros((planes, pset.height // 4, pset.width // 4), dtype=torch.uint8, device=src.device)
    _need(lvl, torch.int32, "tu_pipeline_planes(lvl)")
    _need(rec, torch.int16, "tu_pipeline_planes(rec)")
    _need(tu, torch.uint8, "tu_pipeline_planes(tu)")
    if lvl.numel() < src.numel() or rec.numel() < src.numel() or tu.numel() < planes * (pset.height // 4) * (pset.width // 4):
        raise ValueError("tu_pipeline_planes: output too small")
    check(_lib.load().nh_tu_pipeline_planes(src.data_ptr(), C.byref(pset), int(ctb), int(plane_id), int(seed) & 0xffffffff,
                                            int(qp), int(bool(is_luma)), int(row0), int(min(row1, 1 << 30)),
                                            lvl.data_ptr(), rec.data_ptr(), tu.data_ptr(), C.c_void_p(_stream(stream, src.device))))
    return lvl, rec, tu


def tu_pipeline_planes_compact(src, pset: PlaneSet, ctb: int, plane_id: int, seed: int, qp: int = 32,
                               is_luma: bool = True, row0: int = 0, row1: int = 1 << 30, lvl=None, rec=None, tu=None,
                               spill=None, stream=None):
    """``tu_pipeline_planes`` with COMPACT levels: int16 levels in the source
    layout (exact: |level| <= 408 for an 8-bit TU at every QP and size,
    tools/packed_bounds.py level_bounds) -- 6 instead of 8 bytes per sample.
    Strips with a sample outside [0, 255] (the 32-bit chain) write their int32
    levels into ``spill`` (int32, source layout; allocated uninitialised when
    None) and -32768 at each strip origin.  CTB 16 / 32.  Returns (lvl int16, rec,
    tu, spill); ``tu_levels_widen`` gives the int32 levels of ``tu_pipeline_planes``."""
    torch = _torch()
    _need(src, torch.int16, "tu_pipeline_planes_compact(src)")
    sets_fit_rows([pset], src.numel(), int(row0) * ctb - 1, min(int(row1), 1 << 30) * ctb, "tu_pipeline_planes_compact")
    planes = pset.planes_per_group * pset.num_groups
    if lvl is None:
        lvl = torch.zeros(src.shape, dtype=torch.int16, device=src.device)
    if rec is None:
        rec = torch.zeros(src.shape, dtype=torch.int16, device=src.device)
    if tu is None:
        tu = torch.zeros((planes, pset.height // 4, pset.width // 4), dtype=torch.uint8, device=src.device)
    if spill is None:
        spill = torch.empty(src.shape, dtype=torch.int32, device=src.device)
    _need(lvl, torch.int16, "tu_pipeline_planes_compact(lvl)")
    _need(rec, torch.int16, "tu_pipeline_planes_compact(rec)")
    _need(tu, torch.uint8, "tu_pipeline_planes_compact(tu)")
    _need(spill, torch.int32, "tu_pipeline_planes_compact(spill)")
    if min(lvl.numel(), rec.numel(), spill.numel()) < src.numel() or \
            tu.numel() < planes * (pset.height // 4) * (pset.width // 4):
        raise ValueError("tu_pipeline_planes_compact: output too small")
    check(_lib.load().nh_tu_pipeline_planes_compact(
        src.data_ptr(), C.byref(pset), int(ctb), int(plane_id), int(seed) & 0xffffffff, int(qp), int(bool(is_luma)),
        int(row0), int(min(row1, 1 << 30)), lvl.data_ptr(), spill.data_ptr(), rec.data_ptr(), tu.data_ptr(),
        C.c_void_p(_stream(stream, src.device))), "tu_pipeline_planes_compact")
    return lvl, rec, tu, spill


def tu_levels_widen(lvl, spill, pset: PlaneSet, ctb: int, row0: int = 0, row1: int = 1 << 30, out=None, stream=None):
    """(int16 levels, spill) of ``tu_pipeline_planes_compact`` -> the reference's
    int32 levels of CTU rows [row0, row1) of every plane of ``pset``."""
    torch = _torch()
    _need(lvl, torch.int16, "tu_levels_widen(lvl)")
    _need(spill, torch.int32, "tu_levels_widen(spill)")
    if out is None:
        out = torch.zeros(lvl.shape, dtype=torch.int32, device=lvl.device)
    _need(out, torch.int32, "tu_levels_widen(out)")
    sets_fit_rows([pset], min(lvl.numel(), spill.numel(), out.numel()), int(row0) * ctb,
                  min(int(row1), 1 << 30) * ctb, "tu_levels_widen")
    check(_lib.load().nh_tu_levels_widen(lvl.data_ptr(), spill.data_ptr(), C.byref(pset), int(ctb), int(row0),
                                         int(min(row1, 1 << 30)), out.data_ptr(), C.c_void_p(_stream(stream, lvl.device))),
          "tu_levels_widen")
    return out


def _tu_closed_launch(src, pset: PlaneSet, ctb: int, plane_id: int, seed: int, qp: int, is_luma: bool,
                      lvl, rec, tu, strm):
    """Stream-ordered launch of the config-4 closed loop over one plane set on the
    torch stream ``strm`` (default outputs are zero-filled on that stream too);
    returns (lvl, rec, tu, workspace) -- the workspace holds the wavefront status word."""
    torch = _torch()
    with torch.cuda.device(src.device), torch.cuda.stream(strm):
        return _tu_closed_launch_on(src, pset, ctb, plane_id, seed, qp, is_luma, lvl, rec, tu, int(strm.cuda_stream))


def _tu_closed_launch_on(src, pset, ctb, plane_id, seed, qp, is_luma, lvl, rec, tu, st: int):
    torch = _torch()
    _need(src, torch.int16, "tu_pipeline_closed(src)")
    sets_fit([pset], src.numel(), "tu_pipeline_closed")
    planes = pset.planes_per_group * pset.num_groups
    L = _lib.load()
    wb = int(L.nh_tu_pipeline_closed_workspace_bytes(C.byref(pset), int(ctb)))
    if wb < 0:
        raise ValueError("tu_pipeline_closed: bad plane set (w, h multiples of 4) or CTB size")
    if lvl is None:
        lvl = torch.zeros(src.shape, dtype=torch.int32, device=src.device)
    if rec is None:
        rec = torch.zeros(src.shape, dtype=torch.int16, device=src.device)
    if tu is None:
        tu = torch.zeros((planes, pset.height // 4, pset.width // 4), dtype=torch.uint8, device=src.device)
    _need(lvl, torch.int32, "tu_pipeline_closed(lvl)")
    _need(rec, torch.int16, "tu_pipeline_closed(rec)")
    _need(tu, torch.uint8, "tu_pipeline_closed(tu)")
    if lvl.numel() < src.numel() or rec.numel() < src.numel() or tu.numel() < planes * (pset.height // 4) * (pset.width // 4):
        raise ValueError("tu_pipeline_closed: output too small")
    work = torch.empty((wb + 7) // 8, dtype=torch.int64, device=src.device)
    check(L.nh_tu_pipeline_planes_closed(src.data_ptr(), C.byref(pset), int(ctb), int(plane_id), int(seed) & 0xffffffff,
                                         int(qp), int(bool(is_luma)), lvl.data_ptr(), rec.data_ptr(), tu.data_ptr(),
                                         work.data_ptr(), C.c_void_p(st)), "tu_pipeline_closed")
    return lvl, rec, tu, work


def tu_pipeline_closed(src, pset: PlaneSet, ctb: int, plane_id: int, seed: int, qp: int = 32, is_luma: bool = True,
                       lvl=None, rec=None, tu=None, stream=None):
    """Config 4 in CLOSED loop over every plane of one plane
    set: TUs in z-order with neighbours from the reconstruction, a device
    wavefront over CTU rows.  Returns (lvl int32, recon int16 -- source
    layout, zeros outside every TU --, tu uint8 (planes, h/4, w/4)).
    Speed note: the packed 16-bit plane-pair form runs only when EVERY source
    sample of the set is in [0, 255]; one sample outside sends the whole set to
    the 32-bit form (same results, ~1.7x the time)."""
    torch = _torch()
    strm = stream if stream is not None else torch.cuda.current_stream(src.device)
    st = _stream(strm, src.device)
    lvl, rec, tu, work = _tu_closed_launch(src, pset, ctb, plane_id, seed, qp, is_luma, lvl, rec, tu, strm)
    _closed_status(work, st, "tu_pipeline_closed")
    return lvl, rec, tu


_SIDE_STREAMS = {}


def tu_pipeline_closed_yuv420(src, luma: PlaneSet, chroma: PlaneSet, seed: int, qp: int = 32,
                              lvl=None, rec=None, tu_luma=None, tu_chroma=None, stream=None):
    """Config 4 in closed loop over a YUV420 stream: the luma set (CTB 32,
    plane id 0) and the chroma set (CTB 16, plane ids 1, 2) -- the two calls
    of ``tu_pipeline_closed`` -- run as two concurrent device wavefronts, the
    chroma one on a side stream forked from and joined back into ``stream``.
    One set's CTU rows alone leave most SIMDs with one latency-bound wave
    (DESIGN.md §4.4a).  Same results as the two calls in sequence.
    Returns (lvl, rec, tu_luma, tu_chroma)."""
    torch = _torch()
    dev = src.device
    main = stream if stream is not None else torch.cuda.current_stream(dev)
    if main.device != dev:
        raise ValueError(f"tu_pipeline_closed_yuv420: stream on {main.device} but src on {dev}")
    if not sets_disjoint(luma, chroma):
        # the two wavefronts would write shared lvl / rec elements concurrently: code them in sequence
        lvl, rec, tu_luma = tu_pipeline_closed(src, luma, 32, 0, seed, qp, True, lvl, rec, tu_luma, main)
        lvl, rec, tu_chroma = tu_pipeline_closed(src, chroma, 16, 1, seed, qp, False, lvl, rec, tu_chroma, main)
        return lvl, rec, tu_luma, tu_chroma
    side = _SIDE_STREAMS.get(dev.index)
    if side is None:
        side = _SIDE_STREAMS[dev.index] = torch.cuda.Stream(device=dev)
    with torch.cuda.device(dev), torch.cuda.stream(main):   # default outputs zero-filled in order on `main`
        if lvl is None:
            lvl = torch.zeros(src.shape, dtype=torch.int32, device=dev)
        if rec is None:
            rec = torch.zeros(src.shape, dtype=torch.int16, device=dev)
    fork = torch.cuda.Event()
    fork.record(main)
    side.wait_event(fork)
    # luma first: its wavefront is the critical path and its waves take their slots before chroma's
    # (0.1179 vs 0.1205 ms per 4K frame chroma-first)
    _, _, tu_luma, work_y = _tu_closed_launch(src, luma, 32, 0, seed, qp, True, lvl, rec, tu_luma, main)
    _, _, tu_chroma, work_c = _tu_closed_launch(src, chroma, 16, 1, seed, qp, False, lvl, rec, tu_chroma, side)
    join = torch.cuda.Event()
    join.record(side)
    main.wait_event(join)
    for t in (tu_chroma, work_c):
        t.record_stream(main)
    # one host round trip for both status words: chroma's ORed into a copy of luma's on `main`
    with torch.cuda.device(dev), torch.cuda.stream(main):
        both = work_y[:1].clone()
        both.view(torch.int32)[1:2].bitwise_or_(work_c[:1].view(torch.int32)[1:2])
    try:
        _closed_status(both, int(main.cuda_stream), "tu_pipeline_closed_yuv420")
    except RuntimeError:
        _closed_status(work_y, int(main.cuda_stream), "tu_pipeline_closed_yuv420 (luma)")
        _closed_status(work_c, int(main.cuda_stream), "tu_pipeline_closed_yuv420 (chroma)")
        raise
    return lvl, rec, tu_luma, tu_chroma


def _tu_map_need(t, pset: PlaneSet, dev, what):
    """A per-4x4-unit map of one plane set: uint8, contiguous, on ``dev``, at least
    planes * (h/4) * (w/4) entries; with two or more dimensions its trailing shape
    must be the plane's (h/4, w/4)."""
    torch = _torch()
    _need(t, torch.uint8, what)
    if t.device != dev:
        raise ValueError(f"{what}: on {t.device}, the other tensors on {dev}")
    h4, w4 = pset.height // 4, pset.width // 4
    n = pset.planes_per_group * pset.num_groups * h4 * w4
    if t.numel() < n:
        raise ValueError(f"{what}: {t.numel()} entries for {n} 4x4 units")
    if t.dim() >= 2 and tuple(t.shape[-2:]) != (h4, w4):
        raise ValueError(f"{what}: trailing shape {tuple(t.shape[-2:])}, expected {(h4, w4)}")


def _tu_set_check(pset: PlaneSet, ctb: int, what: str):
    if int(ctb) not in (16, 32):
        raise ValueError(f"{what}: ctb must be 16 or 32")
    if pset.width % 4 or pset.height % 4 or pset.width < 4 or pset.height < 4:
        raise ValueError(f"{what}: width and height must be positive multiples of 4")


def tu_pred_map_closed(src, rec, tu, pset: PlaneSet, ctb: int, pm=None, stream=None):
    """The pred-mode map of a ``tu_pipeline_closed`` call, derived
    after the fact from that call's ``src``, ``rec`` and ``tu``: per TU 1 where the
    encoder chose DC, 0 where it chose planar, written to every 4x4 unit of the TU.
    Every TU is independent (its neighbours are finished reconstruction samples):
    one parallel launch.  Returns pm uint8 (planes, h/4, w/4)."""
    torch = _torch()
    _need(src, torch.int16, "tu_pred_map_closed(src)")
    _need(rec, torch.int16, "tu_pred_map_closed(rec)")
    if rec.device != src.device:
        raise ValueError("tu_pred_map_closed: src and rec on different devices")
    _tu_set_check(pset, ctb, "tu_pred_map_closed")
    sets_fit([pset], min(src.numel(), rec.numel()), "tu_pred_map_closed")
    _tu_map_need(tu, pset, src.device, "tu_pred_map_closed(tu)")
    planes = pset.planes_per_group * pset.num_groups
    if pm is None:
        pm = torch.zeros((planes, pset.height // 4, pset.width // 4), dtype=torch.uint8, device=src.device)
    _tu_map_need(pm, pset, src.device, "tu_pred_map_closed(pm)")
    check(_lib.load().nh_tu_closed_pred_map(src.data_ptr(), rec.data_ptr(), tu.data_ptr(), C.byref(pset), int(ctb),
                                            pm.data_ptr(), C.c_void_p(_stream(stream, src.device))),
          "tu_pred_map_closed")
    return pm


def dequant_inv_tu(lvl, tu, pset: PlaneSet, ctb: int, is_luma: bool = True, qp: int = 32, out=None, stream=None):
    """Stage R of the config-4 decoder: per TU of the map ``tu``
    inverse_transform(dequantize_block(level, qp), use_dst = is_luma and N == 4).astype(int16)
    on the int16 or int32 level planes of ``pset`` inside ``lvl``; exact for every
    level value of the dtype.  The residual lands at the same positions of ``out``
    (int16).  The map is not validated here (``tu_decode_closed`` does): a bad one
    is memory-safe and gives an unspecified residual."""
    out = _dequant_need("dequant_inv_tu", lvl, out)
    _tu_set_check(pset, ctb, "dequant_inv_tu")
    sets_fit([pset], min(lvl.numel(), out.numel()), "dequant_inv_tu")
    _tu_map_need(tu, pset, lvl.device, "dequant_inv_tu(tu)")
    check(_lib.load().nh_dequant_inv_tu_planes(lvl.data_ptr(), lvl.element_size(), out.data_ptr(), tu.data_ptr(),
                                               C.byref(pset), int(ctb), int(bool(is_luma)), int(qp),
                                               C.c_void_p(_stream(stream, lvl.device))), "dequant_inv_tu")
    return out


def _tu_decode_launch(tu, pm, lvl, pset: PlaneSet, ctb: int, is_luma: bool, qp: int, rec, strm):
    """Stream-ordered launch of the config-4 decoder over one plane set on the torch
    stream ``strm``; returns (rec, workspace) -- the workspace holds the status word."""
    torch = _torch()
    _need(lvl, torch.int32, "tu_decode_closed(lvl)")
    _tu_set_check(pset, ctb, "tu_decode_closed")
    sets_fit([pset], lvl.numel(), "tu_decode_closed")
    _tu_map_need(tu, pset, lvl.device, "tu_decode_closed(tu)")
    _tu_map_need(pm, pset, lvl.device, "tu_decode_closed(pm)")
    L = _lib.load()
    wb = int(L.nh_tu_decode_closed_workspace_bytes(C.byref(pset), int(ctb)))
    if wb < 0:
        raise ValueError("tu_decode_closed: bad plane set (w, h multiples of 4) or CTB size")
    with torch.cuda.device(lvl.device), torch.cuda.stream(strm):
        if rec is None:
            rec = torch.zeros(lvl.shape, dtype=torch.int16, device=lvl.device)
        _need(rec, torch.int16, "tu_decode_closed(rec)")
        if rec.device != lvl.device:
            raise ValueError("tu_decode_closed: rec and lvl on different devices")
        if rec.numel() < lvl.numel():
            raise ValueError("tu_decode_closed: rec smaller than lvl")
        work = torch.empty((wb + 7) // 8, dtype=torch.int64, device=lvl.device)
        check(L.nh_tu_decode_planes_closed(tu.data_ptr(), pm.data_ptr(), lvl.data_ptr(), C.byref(pset), int(ctb),
                                           int(bool(is_luma)), int(qp), rec.data_ptr(), work.data_ptr(),
                                           C.c_void_p(int(strm.cuda_stream))), "tu_decode_closed")
    return rec, work


_TU_BAD_MAP = ("bad map (tu is no partition into aligned squares of 4..ctb samples inside the plane, or a pm value "
               "above 1; status 2)")


def tu_decode_closed(tu, pm, lvl, pset: PlaneSet, ctb: int, qp: int = 32, is_luma: bool = True, rec=None,
                     stream=None):
    """The decoder of ``tu_pipeline_closed``: from that call's
    ``tu`` and ``lvl`` (int32, source layout), the pred-mode map ``pm`` of
    ``tu_pred_map_closed``, ``pset``, ``ctb``, ``qp`` and ``is_luma`` rebuild its
    reconstruction: stage R, then one prediction per TU in closed loop on the
    CTU-row wavefront.  Map-driven: any ``tu`` that partitions every plane into
    aligned squares of 4..ctb samples decodes, whatever made it; any other map, or
    a ``pm`` value above 1, raises ValueError (``rec`` is then unspecified).
    Returns recon int16 (source layout)."""
    torch = _torch()
    if not isinstance(lvl, torch.Tensor) or not lvl.is_cuda:
        raise TypeError("tu_decode_closed(lvl): expected a CUDA/HIP torch tensor")
    strm = stream if stream is not None else torch.cuda.current_stream(lvl.device)
    st = _stream(strm, lvl.device)
    rec, work = _tu_decode_launch(tu, pm, lvl, pset, ctb, is_luma, qp, rec, strm)
    _closed_status(work, st, "tu_decode_closed", _TU_BAD_MAP)
    return rec


def tu_decode_closed_yuv420(tu_luma, pm_luma, tu_chroma, pm_chroma, lvl, luma: PlaneSet, chroma: PlaneSet,
                            qp: int = 32, rec=None, stream=None):
    """The decoder of ``tu_pipeline_closed_yuv420``: the luma set (CTB 32) and the
    chroma set (CTB 16) -- the two calls of ``tu_decode_closed`` -- as two concurrent
    device wavefronts, the chroma one on a side stream forked from and joined back
    into ``stream``; in sequence when the sets share elements.  Returns rec."""
    torch = _torch()
    if not isinstance(lvl, torch.Tensor) or not lvl.is_cuda:
        raise TypeError("tu_decode_closed_yuv420(lvl): expected a CUDA/HIP torch tensor")
    dev = lvl.device
    main = stream if stream is not None else torch.cuda.current_stream(dev)
    if main.device != dev:
        raise ValueError(f"tu_decode_closed_yuv420: stream on {main.device} but lvl on {dev}")
    if not sets_disjoint(luma, chroma):
        # the two wavefronts would write shared rec elements concurrently: decode them in sequence
        rec = tu_decode_closed(tu_luma, pm_luma, lvl, luma, 32, qp, True, rec, main)
        return tu_decode_closed(tu_chroma, pm_chroma, lvl, chroma, 16, qp, False, rec, main)
    side = _SIDE_STREAMS.get(dev.index)
    if side is None:
        side = _SIDE_STREAMS[dev.index] = torch.cuda.Stream(device=dev)
    if rec is None:
        with torch.cuda.device(dev), torch.cuda.stream(main):
            rec = torch.zeros(lvl.shape, dtype=torch.int16, device=dev)
    fork = torch.cuda.Event()
    fork.record(main)
    side.wait_event(fork)
    work_y = work_c = None
    try:
        # luma first: its wavefront is the longer one and takes its slots before chroma's
        rec, work_y = _tu_decode_launch(tu_luma, pm_luma, lvl, luma, 32, True, qp, rec, main)
        _, work_c = _tu_decode_launch(tu_chroma, pm_chroma, lvl, chroma, 16, False, qp, rec, side)
    finally:   # whatever was queued on the side stream is joined back, also when a check raised
        join = torch.cuda.Event()
        join.record(side)
        main.wait_event(join)
        if work_c is not None:
            work_c.record_stream(main)
    # one host round trip for both status words: chroma's ORed into a copy of luma's on `main`
    with torch.cuda.device(dev), torch.cuda.stream(main):
        both = work_y[:1].clone()
        both.view(torch.int32)[1:2].bitwise_or_(work_c[:1].view(torch.int32)[1:2])
    try:
        _closed_status(both, int(main.cuda_stream), "tu_decode_closed_yuv420", _TU_BAD_MAP)
    except (ValueError, RuntimeError):   # name the set; a bad map (status 2) goes before a stall (status 1)
        errs = []
        for work, name in ((work_y, "luma"), (work_c, "chroma")):
            try:
                _closed_status(work, int(main.cuda_stream), "tu_decode_closed_yuv420 (%s)" % name, _TU_BAD_MAP)
            except (ValueError, RuntimeError) as e:
                errs.append(e)
        for e in sorted(errs, key=lambda e: not isinstance(e, ValueError)):
            raise e
        raise
    return rec


def _tu_rd_prepare(src, pset: PlaneSet, ctb: int, qp: int, lam: int, lvl, rec, what: str):
    """Argument checks and default outputs shared by the search and the map-driven
    encode; returns (lvl, rec, planes)."""
    torch = _torch()
    _need(src, torch.int16, f"{what}(src)")
    _tu_set_check(pset, ctb, what)
    if not 0 <= int(qp) <= 51:
        raise ValueError(f"{what}: qp must be in 0..51")
    if not 0 <= int(lam) <= 2 ** 31 - 1:
        raise ValueError(f"{what}: lam must be in 0..2^31-1")
    sets_fit([pset], src.numel(), what)
    dev = src.device
    if lvl is None:
        lvl = torch.zeros(src.shape, dtype=torch.int32, device=dev)
    if rec is None:
        rec = torch.zeros(src.shape, dtype=torch.int16, device=dev)
    _need(lvl, torch.int32, f"{what}(lvl)")
    _need(rec, torch.int16, f"{what}(rec)")
    if lvl.device != dev or rec.device != dev:
        raise ValueError(f"{what}: lvl / rec and src on different devices")
    sets_fit([pset], min(lvl.numel(), rec.numel()), f"{what}(lvl, rec)")
    return lvl, rec, pset.planes_per_group * pset.num_groups


def tu_rd_planes(src, pset: PlaneSet, ctb: int, qp: int = 32, lam: int = 0, is_luma: bool = True, lvl=None, rec=None,
                 tu=None, pm=None, stream=None):
    """Config 4 with the quadtree CHOSEN by integer RD cost, open loop (DESIGN.md
    §3.4a), over every plane of one plane set: every aligned candidate TU of every
    size 4..ctb runs §3.4's chain (neighbours from the source, 128 outside the
    plane), J = D + lam * R with D = sum (int16)(orig - rec)^2 and R =
    count_nonzero(level) + 1; bottom-up per CTB a node becomes one TU iff its J <=
    the sum of its four best children (the parent wins ties, a node that overhangs
    the plane splits).  ``ctb`` 16 or 32, ``qp`` 0..51, ``lam`` 0..2^31-1.
    Returns (lvl int32, rec int16 -- source layout --, tu uint8 log2 TU size, pm
    uint8 1 = DC / 0 = planar -- (planes, h/4, w/4) --, stats int64 (planes, 3):
    sum J, sum D, sum R over the plane's TUs)."""
    torch = _torch()
    lvl, rec, planes = _tu_rd_prepare(src, pset, ctb, qp, lam, lvl, rec, "tu_rd_planes")
    dev = src.device
    shape = (planes, pset.height // 4, pset.width // 4)
    if tu is None:
        tu = torch.zeros(shape, dtype=torch.uint8, device=dev)
    if pm is None:
        pm = torch.zeros(shape, dtype=torch.uint8, device=dev)
    _tu_map_need(tu, pset, dev, "tu_rd_planes(tu)")
    _tu_map_need(pm, pset, dev, "tu_rd_planes(pm)")
    stats = torch.empty((planes, 3), dtype=torch.int64, device=dev)
    check(_lib.load().nh_tu_rd_planes(src.data_ptr(), C.byref(pset), int(ctb), int(qp), int(bool(is_luma)), int(lam),
                                      lvl.data_ptr(), rec.data_ptr(), tu.data_ptr(), pm.data_ptr(), stats.data_ptr(),
                                      C.c_void_p(_stream(stream, dev))), "tu_rd_planes")
    return lvl, rec, tu, pm, stats


def tu_rd_plane(src2d, ctb: int, qp: int = 32, lam: int = 0, is_luma: bool = True, stream=None):
    """``tu_rd_planes`` on one int16 plane (H, W).  Returns (lvl (H, W), rec (H, W),
    tu (H/4, W/4), pm (H/4, W/4), stats (3,))."""
    torch = _torch()
    _need(src2d, torch.int16, "tu_rd_plane")
    if src2d.dim() != 2:
        raise ValueError("tu_rd_plane: expected a 2-D plane")
    h, w = src2d.shape
    lvl, rec, tu, pm, stats = tu_rd_planes(src2d, plane_set(0, w, h, w), ctb, qp, lam, is_luma, stream=stream)
    return lvl, rec, tu[0], pm[0], stats[0]


def tu_encode_map_planes(src, tu, pset: PlaneSet, ctb: int, qp: int = 32, lam: int = 0, is_luma: bool = True,
                         lvl=None, rec=None, pm=None, stream=None):
    """Config 4 on a quadtree the CALLER supplies, open loop: every
    TU of the map ``tu`` (uint8 log2 TU size per 4x4 unit, (planes, h/4, w/4)) runs
    §3.4's chain once at its size.  Map-driven: any ``tu`` that partitions every plane
    into aligned squares of 4..ctb samples is coded, whatever made it; any other map
    raises ValueError (the outputs are then unspecified).  ``lam`` enters only
    ``stats``.  Returns (lvl, rec, pm, stats) as ``tu_rd_planes``."""
    torch = _torch()
    lvl, rec, planes = _tu_rd_prepare(src, pset, ctb, qp, lam, lvl, rec, "tu_encode_map_planes")
    dev = src.device
    _tu_map_need(tu, pset, dev, "tu_encode_map_planes(tu)")
    if pm is None:
        pm = torch.zeros((planes, pset.height // 4, pset.width // 4), dtype=torch.uint8, device=dev)
    _tu_map_need(pm, pset, dev, "tu_encode_map_planes(pm)")
    stats = torch.empty((planes, 3), dtype=torch.int64, device=dev)
    L = _lib.load()
    work = torch.empty((int(L.nh_tu_encode_map_workspace_bytes()) + 7) // 8, dtype=torch.int64, device=dev)
    st = _stream(stream, dev)
    check(L.nh_tu_encode_map_planes(src.data_ptr(), tu.data_ptr(), C.byref(pset), int(ctb), int(qp), int(bool(is_luma)),
                                    int(lam), lvl.data_ptr(), rec.data_ptr(), pm.data_ptr(), stats.data_ptr(),
                                    work.data_ptr(), C.c_void_p(st)), "tu_encode_map_planes")
    if planes:
        status = C.c_int(0)
        check(L.nh_intra_rdo_closed_status(work.data_ptr(), C.byref(status), C.c_void_p(st)))
        if status.value:
            raise ValueError("tu_encode_map_planes: bad map (tu is no partition into aligned squares of 4..ctb "
                             "samples inside the plane; status %d)" % status.value)
    return lvl, rec, pm, stats


def tu_rd_yuv420(src, luma: PlaneSet, chroma: PlaneSet, qp: int = 32, lam: int = 0, lvl=None, rec=None, stream=None):
    """``tu_rd_planes`` over a YUV420 stream: the luma set with CTB 32 and the DST, the
    U+V set with CTB 16 and without it (the pairing of ``tu_pipeline_closed_yuv420``),
    in sequence on one stream into shared ``lvl`` / ``rec``.
    Returns (lvl, rec, (tu, pm, stats) of luma, (tu, pm, stats) of chroma)."""
    lvl, rec, tu_y, pm_y, st_y = tu_rd_planes(src, luma, 32, qp, lam, True, lvl, rec, stream=stream)
    lvl, rec, tu_c, pm_c, st_c = tu_rd_planes(src, chroma, 16, qp, lam, False, lvl, rec, stream=stream)
    return lvl, rec, (tu_y, pm_y, st_y), (tu_c, pm_c, st_c)


_PIPE_STREAMS = {}


def tu_pipeline_closed_yuv420_stream(src, width: int, height: int, num_frames: int, seed: int, qp: int = 32,
                                     batch_frames: int = 128, depth: int = 3, lvl=None, rec=None, tu_luma=None,
                                     tu_chroma=None, stream=None, frame_stride: int | None = None, base: int = 0):
    """Config 4 in closed loop over a stream of YUV420 frames laid out back to
    back (PackedFrame layout, as ``yuv420_plane_sets``): batches of
    ``batch_frames`` frames, each batch's luma and chroma wavefronts
    (``tu_pipeline_closed_yuv420``) on a stream pair of their own, ``depth``
    pairs in rotation, so up to ``depth`` batches are in flight: a batch's CTU
    rows fill the SIMDs that the previous batch's wavefront leaves idle while it
    ramps down (4K: 0.048-0.049 ms per frame with the defaults,
    0.054-0.055 with 64-frame batches, vs 0.065-0.068 for one 64-frame call).
    No host round trip between batches; one status check at the end.  Same results as one ``tu_pipeline_closed_yuv420``
    call over all the frames (frames are independent).
    Returns (lvl, rec, tu_luma (num_frames, h/4, w/4), tu_chroma (2 num_frames, h/8, w/8))."""
    torch = _torch()
    if batch_frames < 1 or depth < 1 or num_frames < 0:
        raise ValueError("tu_pipeline_closed_yuv420_stream: batch_frames, depth >= 1 and num_frames >= 0")
    fs = frame_stride or yuv420_frame_elems(width, height)
    if fs < yuv420_frame_elems(width, height):
        raise ValueError("tu_pipeline_closed_yuv420_stream: frame_stride shorter than a frame")
    sets_fit(yuv420_plane_sets(num_frames, width, height, fs, base), src.numel(), "tu_pipeline_closed_yuv420_stream")
    dev = src.device
    main = stream if stream is not None else torch.cuda.current_stream(dev)
    if main.device != dev:
        raise ValueError(f"tu_pipeline_closed_yuv420_stream: stream on {main.device} but src on {dev}")
    with torch.cuda.device(dev), torch.cuda.stream(main):   # outputs zero-filled in order on `main`, before the fork
        if lvl is None:
            lvl = torch.zeros(src.shape, dtype=torch.int32, device=dev)
        if rec is None:
            rec = torch.zeros(src.shape, dtype=torch.int16, device=dev)
        if tu_luma is None:
            tu_luma = torch.zeros((num_frames, height // 4, width // 4), dtype=torch.uint8, device=dev)
        if tu_chroma is None:
            tu_chroma = torch.zeros((2 * num_frames, height // 8, width // 8), dtype=torch.uint8, device=dev)
    for t, what, n in ((tu_luma, "tu_luma", num_frames), (tu_chroma, "tu_chroma", 2 * num_frames)):
        if not t.is_contiguous() or t.dim() != 3 or t.shape[0] < n:
            raise ValueError(f"tu_pipeline_closed_yuv420_stream: {what} must be a contiguous (>= {n}, h, w) tensor")
    if num_frames == 0:
        return lvl, rec, tu_luma, tu_chroma
    pool = _PIPE_STREAMS.setdefault(dev.index, [])
    while len(pool) < depth:
        pool.append((torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)))
    fork = torch.cuda.Event()
    fork.record(main)
    for pair in pool[:depth]:
        for s_ in pair:
            s_.wait_event(fork)
    works = []
    for b, f0 in enumerate(range(0, num_frames, batch_frames)):
        nb = min(batch_frames, num_frames - f0)
        sy, suv = yuv420_plane_sets(nb, width, height, fs, base + f0 * fs)
        ls, cs = pool[b % depth]
        works.append(_tu_closed_launch(src, sy, 32, 0, seed, qp, True, lvl, rec, tu_luma[f0:f0 + nb], ls)[3])
        works.append(_tu_closed_launch(src, suv, 16, 1, seed, qp, False, lvl, rec,
                                       tu_chroma[2 * f0:2 * (f0 + nb)], cs)[3])
    for pair in pool[:depth]:
        for s_ in pair:
            join = torch.cuda.Event()
            join.record(s_)
            main.wait_event(join)
    for w_ in works:
        w_.record_stream(main)
    with torch.cuda.device(dev), torch.cuda.stream(main):   # every status word ORed: one host round trip
        both = works[0][:1].clone()
        for w_ in works[1:]:
            both.view(torch.int32)[1:2].bitwise_or_(w_[:1].view(torch.int32)[1:2])
    try:
        _closed_status(both, int(main.cuda_stream), "tu_pipeline_closed_yuv420_stream")
    except RuntimeError:
        for k, w_ in enumerate(works):
            _closed_status(w_, int(main.cuda_stream),
                              f"tu_pipeline_closed_yuv420_stream (batch {k // 2}, {'chroma' if k % 2 else 'luma'})")
        raise
    return lvl, rec, tu_luma, tu_chroma


def tc32_plane(src, qp: int = 32, variant: int = 1, lvl=None, rec=None, stream=None):
    """Config 5 on one int16 plane (H, W), W % 8 == 0: every full
    32x32 block through the chain.  variant 0 = butterfly, 1 = matrix cores (f16
    for 8-bit blocks, int8 otherwise), 2 = int8 MFMA only (A/B).
    Returns (levels int32 (H, W), recon int16 (H, W))."""
    torch = _torch()
    _need(src, torch.int16, "tc32_plane")
    h, w = src.shape
    lvl = torch.zeros((h, w), dtype=torch.int32, device=src.device) if lvl is None else lvl
    rec = torch.zeros((h, w), dtype=torch.int16, device=src.device) if rec is None else rec
    check(_lib.load().nh_tc32_plane(src.data_ptr(), w, h, w, int(qp), lvl.data_ptr(), rec.data_ptr(), int(variant),
                                    C.c_void_p(_stream(stream, src.device))), "tc32_plane")
    return lvl, rec


def tc32_planes(src, sets, qp: int = 32, variant: int = 1, lvl=None, rec=None, stream=None):
    """Config 5 over every plane of ``sets`` (e.g. yuv420_plane_sets of a frame
    stream): per plane set one f16-MFMA launch plus an int8 fix-up for non-8-bit
    blocks (variant 1), one int8-MFMA launch (2), or the butterfly
    per plane (variant 0).  Returns (levels int32, recon int16), source layout."""
    torch = _torch()
    _need(src, torch.int16, "tc32_planes(src)")
    sets_fit(sets, src.numel(), "tc32_planes")
    if lvl is None:
        lvl = torch.zeros(src.shape, dtype=torch.int32, device=src.device)
    if rec is None:
        rec = torch.zeros(src.shape, dtype=torch.int16, device=src.device)
    _need(lvl, torch.int32, "tc32_planes(lvl)")
    _need(rec, torch.int16, "tc32_planes(rec)")
    if lvl.numel() < src.numel() or rec.numel() < src.numel():
        raise ValueError("tc32_planes: lvl / rec smaller than src")
    arr = _set_array(sets)
    check(_lib.load().nh_tc32_planes(src.data_ptr(), arr, len(sets), int(qp), lvl.data_ptr(), rec.data_ptr(),
                                     int(variant), C.c_void_p(_stream(stream, src.device))), "tc32_planes")
    return lvl, rec


def tc32_planes_compact(src, sets, qp: int = 32, level_dtype=None, lvl=None, rec=None, spill=None, stream=None):
    """Config 5 (variant 1) with COMPACT levels: int16 (default) or int8 levels in
    the source layout -- exact, an 8-bit block's 32x32 levels satisfy |level| <= 51
    at every QP (tools/packed_bounds.py level_bounds) -- 6 / 5 bytes per sample of
    traffic instead of 8.  A block that is not 8-bit writes its int32 levels into
    ``spill`` (int32, source layout; allocated uninitialised when None) and the
    marker -32768 / -128 at its compact origin.  Returns (lvl, rec, spill);
    ``tc32_levels_widen(lvl, spill, sets)`` gives the int32 levels of
    ``tc32_planes``."""
    torch = _torch()
    _need(src, torch.int16, "tc32_planes_compact(src)")
    sets_fit(sets, src.numel(), "tc32_planes_compact")
    dt = level_dtype if level_dtype is not None else (lvl.dtype if lvl is not None else torch.int16)
    if dt not in (torch.int16, torch.int8):
        raise TypeError("tc32_planes_compact: level_dtype must be torch.int16 or torch.int8")
    if lvl is None:
        lvl = torch.zeros(src.shape, dtype=dt, device=src.device)
    if rec is None:
        rec = torch.zeros(src.shape, dtype=torch.int16, device=src.device)
    if spill is None:
        spill = torch.empty(src.shape, dtype=torch.int32, device=src.device)
    _need(lvl, dt, "tc32_planes_compact(lvl)")
    _need(rec, torch.int16, "tc32_planes_compact(rec)")
    _need(spill, torch.int32, "tc32_planes_compact(spill)")
    if min(lvl.numel(), rec.numel(), spill.numel()) < src.numel():
        raise ValueError("tc32_planes_compact: lvl / rec / spill smaller than src")
    arr = _set_array(sets)
    check(_lib.load().nh_tc32_planes_compact(src.data_ptr(), arr, len(sets), int(qp), lvl.data_ptr(),
                                             lvl.element_size(), spill.data_ptr(), rec.data_ptr(),
                                             C.c_void_p(_stream(stream, src.device))), "tc32_planes_compact")
    return lvl, rec, spill


def tc32_levels_widen(lvl, spill, sets, out=None, stream=None):
    """(compact levels, spill) of ``tc32_planes_compact`` -> the reference's int32
    levels at every sample of every full 32x32 block (other samples of ``out``
    are left as they are: zeros by default, as ``tc32_planes``)."""
    torch = _torch()
    if not isinstance(lvl, torch.Tensor) or lvl.dtype not in (torch.int16, torch.int8):
        raise TypeError("tc32_levels_widen: lvl must be an int16 / int8 device tensor")
    _need(lvl, lvl.dtype, "tc32_levels_widen(lvl)")
    _need(spill, torch.int32, "tc32_levels_widen(spill)")
    if out is None:
        out = torch.zeros(lvl.shape, dtype=torch.int32, device=lvl.device)
    _need(out, torch.int32, "tc32_levels_widen(out)")
    sets_fit(sets, min(lvl.numel(), spill.numel(), out.numel()), "tc32_levels_widen")
    arr = _set_array(sets)
    check(_lib.load().nh_tc32_levels_widen(lvl.data_ptr(), lvl.element_size(), spill.data_ptr(), arr, len(sets),
                                           out.data_ptr(), C.c_void_p(_stream(stream, lvl.device))),
          "tc32_levels_widen")
    return out


# ---------------------------------------------------------------------------
# Frame I/O (frame.py:44-54, :87-115, :176-183) and the frame-level intra
# driver (__main__.py:142-189) -- SURVEY.md §8(f) f-3 / f-1.
# ---------------------------------------------------------------------------
ENC_STATS = 6   # blocks, dc wins, planar wins, dc energy, planar energy, uint8 SSE


def widen_u8(src, out=None, stream=None):
    """uint8 samples (e.g. YUV420p bytes uploaded as-is) -> int16, i.e.
    Plane.from_buffer(..).data.astype(np.int16) for every plane at once."""
    torch = _torch()
    _need(src, torch.uint8, "widen_u8(src)")
    if out is None:
        out = torch.empty(src.shape, dtype=torch.int16, device=src.device)
    _need(out, torch.int16, "widen_u8(out)")
    if out.numel() != src.numel():
        raise ValueError("widen_u8: size mismatch")
    check(_lib.load().nh_widen_u8_i16(src.data_ptr(), out.data_ptr(), src.numel(), C.c_void_p(_stream(stream, src.device))))
    return out


def narrow_u8(src, out=None, stream=None):
    """int16 -> uint8 keeping the low byte: numpy's .astype(np.uint8) as used by
    Frame.to_yuv420p / PackedFrame.to_yuv420p."""
    torch = _torch()
    _need(src, torch.int16, "narrow_u8(src)")
    if out is None:
        out = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
    _need(out, torch.uint8, "narrow_u8(out)")
    if out.numel() != src.numel():
        raise ValueError("narrow_u8: size mismatch")
    check(_lib.load().nh_narrow_i16_u8(src.data_ptr(), out.data_ptr(), src.numel(), C.c_void_p(_stream(stream, src.device))))
    return out


def luma_block_size(block_size: int) -> int:
    """encode_frame_intra's luma block: block_size, at least 4 (__main__.py:156-158)."""
    return max(4, block_size)


def chroma_block_size(block_size: int) -> int:
    """encode_frame_intra's chroma block: block_size // 2, at least 4 (__main__.py:156-158)."""
    return max(4, block_size // 2)


def _check_block_size(bs: int):
    if not 1 <= bs <= 65536:
        raise ValueError(f"block size {bs}: the device driver takes 1..65536")


def encode_intra_planes(src, sets: Sequence[PlaneSet], block_sizes: Sequence[int], recon=None, recon_u8=None,
                        stats=None, stream=None):
    """The per-block decision of encode_frame_intra over every plane of ``sets``
    inside ``src`` (uint8 or int16), any block size >= 1.  Returns the
    (accumulated) int64 stats tensor, one ENC_STATS row per plane, planes
    numbered set by set.  Raises OverflowError where the reference's planar
    store does (int16 samples at a block size that is not a power of two: the
    call then waits for the launch to read the status word)."""
    torch = _torch()
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype not in (torch.uint8, torch.int16):
        raise TypeError("encode_intra_planes(src): expected a uint8 or int16 device tensor")
    if not src.is_contiguous():
        raise ValueError("encode_intra_planes(src): tensor must be contiguous")
    for bs in block_sizes:
        _check_block_size(int(bs))
    if len(block_sizes) != len(sets):
        raise ValueError("encode_intra_planes: one block size per plane set")
    nplanes = sum(s.planes_per_group * s.num_groups for s in sets)
    sets_fit(sets, src.numel(), "encode_intra_planes")
    if stats is None:
        stats = torch.zeros((nplanes, ENC_STATS), dtype=torch.int64, device=src.device)
    _need(stats, torch.int64, "encode_intra_planes(stats)")
    if stats.numel() < nplanes * ENC_STATS:
        raise ValueError("encode_intra_planes: stats too small")
    for t, dt, nm in ((recon, torch.int16, "recon"), (recon_u8, torch.uint8, "recon_u8")):
        if t is not None:
            _need(t, dt, f"encode_intra_planes({nm})")
            if t.numel() < src.numel():
                raise ValueError(f"encode_intra_planes: {nm} smaller than src")
    arr = _set_array(sets)
    bsz = (C.c_int32 * len(sets))(*[int(b) for b in block_sizes])
    wide = src.dtype == torch.int16 and any(int(b) & (int(b) - 1) or int(b) < 4 or int(b) > 64 for b in block_sizes)
    status = torch.zeros(1, dtype=torch.int32, device=src.device) if wide else None
    strm = stream if stream is not None else torch.cuda.current_stream(src.device)
    check(_lib.load().nh_encode_intra_planes(
        src.data_ptr(), int(src.dtype == torch.uint8), arr, len(sets), bsz,
        recon.data_ptr() if recon is not None else None, recon_u8.data_ptr() if recon_u8 is not None else None,
        stats.data_ptr(), status.data_ptr() if status is not None else None,
        C.c_void_p(_stream(strm, src.device))))
    if status is not None:
        strm.synchronize()   # the launch's stream only (it may not be torch's current one), not the whole device
    if status is not None and int(status.item()):
        raise OverflowError("encode_intra_planes: planar prediction out of bounds for int16 (intra.py:111)")
    return stats


def encode_intra_yuv420(frames, width: int, height: int, block_size: int, recon=None, recon_u8=None,
                        stream=None):
    """encode_frame_intra (__main__.py:142-189) on a stream of YUV420p frames laid
    out back to back in ``frames`` (uint8 bytes straight from a .yuv file, or
    int16 samples).  Returns stats as an int64 tensor (F, 3, ENC_STATS) for
    the Y, U and V planes of every frame; ``recon`` (int16) / ``recon_u8``
    (to_yuv420p bytes) receive the reconstruction when given."""
    fe = yuv420_frame_elems(width, height)
    if frames.numel() % fe:
        raise ValueError("encode_intra_yuv420: size is not a whole number of frames")
    nf = frames.numel() // fe
    sets = yuv420_plane_sets(nf, width, height)
    st = encode_intra_planes(frames, sets, [luma_block_size(block_size), chroma_block_size(block_size)], recon,
                             recon_u8, stream=stream)
    y, uv = st[:nf], st[nf:].view(nf, 2, ENC_STATS)
    return _torch().cat([y.view(nf, 1, ENC_STATS), uv], 1)


# ---------------------------------------------------------------------------
# block-call server controls (per-block drop-in calls)
# ---------------------------------------------------------------------------
def block_server_stop() -> None:
    """Ask every resident block-call server to leave now and wait until it has
    (a device-wide synchronize then no longer waits for its idle time)."""
    check(_lib.load().nh_block_server_stop(), "block_server_stop")


def block_server_set_idle_us(us: int) -> None:
    """Idle time (us) a server stays resident without a request; 0 = no server
    (every per-block call is its own kernel launch)."""
    check(_lib.load().nh_block_server_set_idle_us(int(us)), "block_server_set_idle_us")


def block_server_stats(device: int = 0) -> dict:
    out = (C.c_int64 * 4)()
    check(_lib.load().nh_block_server_stats(int(device), out), "block_server_stats")
    return {"served": out[0], "launches": out[1], "kernel_calls": out[2], "idle_us": out[3]}
