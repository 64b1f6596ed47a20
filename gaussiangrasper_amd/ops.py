"""Host-side mirror of the gsplat-0.1.0 operator surface the reference model calls
(nerfstudio/models/gaussian_splatting.py:46-50 imports, :699/:730/:735/:747/:759/:773 calls),
sitting directly on the C ABI of libgg_raster.so (include/gg_raster.h).

Same class names, positional argument order, return shapes and error behaviour as
gsplat.project_gaussians.ProjectGaussians, gsplat.sh.SphericalHarmonics,
gsplat.rasterize.RasterizeGaussians and gsplat.nd_rasterize.NDRasterizeGaussians.
PyTorch is plumbing here: it owns device memory and the stream; every kernel is ours.

No CPU path: tensors must live on a HIP device ("cuda" in PyTorch-ROCm), otherwise the operators
raise.  One design difference from the reference, invisible to the caller: the four rasterize
calls of one view share ONE binning (tile sort), cached on the identity+version of
(xys, depths, radii, num_tiles_hit) — the reference re-sorts in every call.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

from . import _lib
from ._call import (f32 as _f32, i32 as _i32, ptr as _ptr, require_hip as _require_hip,  # noqa: F401
                    stream as _stream, workspace as _workspace)
from .constants import BLOCK, CLIP_THRESH_DEFAULT, deg_from_sh, num_sh_bases  # noqa: F401


# ------------------------------------------------------------------------------------------------
# direct gradient accumulation (opt-in; used by dist.GradBucket)
# ------------------------------------------------------------------------------------------------
# Over the views of an optimizer step autograd adds every view's parameter gradient into `.grad`: for
# the two large parameters — SH coefficients (300 B per Gaussian) and features (128 B) — that is a
# freshly written gradient tensor plus a separate read-modify-write add per view.  When the caller has
# registered a persistent gradient buffer for a leaf parameter that enters an operator directly
# (`colors_all` into SphericalHarmonics, `feature` into NDRasterizeGaussians, as at reference
# :730,:747-753), the backward kernel adds into that buffer itself and returns no gradient for the
# input.  Off unless a sink is registered: plain autograd semantics otherwise.
class KeptView(NamedTuple):
    """A view's SH gradient as its factors (12 B per Gaussian), waiting to be expanded into the sink's buffer."""
    degrees_to_use: int
    num_bases: int
    viewdirs: Tensor
    v_rgb: Tensor           # the colour cotangent, clamp mask applied


_grad_sinks = {}        # id(param) -> GradSink
_kept_sh = {}           # id(param) -> [KeptView, ...] of one (degrees_to_use, num_bases); outlives a re-registration


class GradSink:
    """Where the backward kernels add the gradient of leaf `param` (register_grad_sink)."""
    __slots__ = ("param", "buffer", "notify", "defer")

    def __init__(self, param: Tensor, buffer: Tensor, notify=None, defer=None):
        self.param, self.buffer, self.notify, self.defer = param, buffer, notify, defer

    def done(self) -> None:
        """An accumulation into `buffer` has been enqueued."""
        if self.notify is not None:
            self.notify(self.param)

    def keeps_sh(self) -> bool:
        """Keep a view's SH gradient as its factors (or add it now): while more views follow or something is kept."""
        return self.defer is not None and (self.defer() or bool(_kept_sh.get(id(self.param))))

    def keep_sh(self, degrees_to_use: int, num_bases: int, viewdirs: Tensor, v_rgb: Tensor) -> None:
        """Keep one view; views kept with another degree or basis count are expanded first (one expansion takes one),
        everything when no view follows (no `defer`: ViewGeometry's one kernel leaves factors and always comes here)."""
        kept = _kept_sh.get(id(self.param))
        if kept and (kept[0].degrees_to_use, kept[0].num_bases) != (degrees_to_use, num_bases):
            flush_grad_sinks()
        _kept_sh.setdefault(id(self.param), []).append(KeptView(degrees_to_use, num_bases, viewdirs, v_rgb))
        if self.defer is None or not self.defer():
            flush_grad_sinks()


def register_grad_sink(param: Tensor, buffer: Tensor, notify=None, defer=None) -> None:
    """Let the backward kernels accumulate the gradient of leaf `param` straight into `buffer`
    (same shape, fp32, contiguous); `notify(param)` is called after each accumulation is enqueued.
    `defer` (SH coefficients through ShadeTail only): a callable telling whether MORE contributions to this buffer
    will follow before it is read (the caller is in the middle of the views of an optimizer step).  While it
    returns True the operator keeps a view's SH gradient as its factors (12 B per Gaussian) instead of adding
    300 B per Gaussian into the buffer, and expands all kept views in one pass when it returns False — or when
    `flush_grad_sinks()` is called.  `notify` then fires once, after the expansion."""
    if not (param.is_leaf and param.requires_grad):
        raise ValueError("a gradient sink needs a leaf tensor that requires grad")
    if buffer.shape != param.shape or buffer.dtype != torch.float32 or not buffer.is_contiguous():
        raise ValueError("sink buffer must be a contiguous fp32 tensor of the parameter's shape")
    _grad_sinks[id(param)] = GradSink(param, buffer, notify, defer)


def clear_grad_sinks() -> None:
    _grad_sinks.clear()
    _kept_sh.clear()


def discard_deferred_grads() -> None:
    """Forget kept-but-not-expanded contributions (the caller zeroes the gradients they belong to)."""
    _kept_sh.clear()


def flush_grad_sinks() -> None:
    """Expand every kept SH contribution into its buffer now (gg_sh_bwd_multi) and fire the sinks' `notify`."""
    for key in list(_kept_sh):
        kept = _kept_sh.pop(key)
        sink = _grad_sinks.get(key)
        if sink is None or not kept:
            continue
        buf = sink.buffer
        views = (C.c_void_p * len(kept))(*[_ptr(v.viewdirs) for v in kept])
        v_rgbs = (C.c_void_p * len(kept))(*[_ptr(v.v_rgb) for v in kept])
        _lib.check(_lib.load().gg_sh_bwd_multi(buf.shape[0], kept[0].num_bases, kept[0].degrees_to_use, len(kept),
                                               views, v_rgbs, _ptr(buf), 1, _stream(buf.device)), "gg_sh_bwd_multi")
        sink.done()


def _dense_f32(t: Tensor) -> bool:
    return t.dtype == torch.float32 and t.is_contiguous()


def _sink_for(t: Tensor, eligible: bool = True) -> Optional[GradSink]:
    """The sink registered for this very tensor, where the calling operator can add into one (`eligible`)."""
    hit = _grad_sinks.get(id(t)) if eligible else None
    return hit if hit is not None and hit.param is t else None


def _sinks_for_all(*tensors: Tensor):
    """The sinks of fp32 contiguous tensors, all of them or None: one accumulate switch for the kernel."""
    sinks = [_sink_for(t, _dense_f32(t)) for t in tensors]
    return sinks if all(k is not None for k in sinks) else None


# ------------------------------------------------------------------------------------------------
# intersection count: started right after the projection, read when the first rasterize call needs it
# ------------------------------------------------------------------------------------------------
# The reference reads the cumulative tile count with `.item()` inside every rasterize call (SURVEY
# a5): a full host<->device round trip with the GPU idle while the host then enqueues the sort.  Here
# the count kernel and an async copy to pinned memory are enqueued at the end of
# ProjectGaussians.forward, followed by an event; whatever the caller enqueues next (SH, activations)
# keeps the GPU busy, and bin_and_sort_gaussians only waits on that event.
_PIN_SLOTS = 64
_pin_ring = {}          # device index -> (pinned int64[_PIN_SLOTS], next slot)
_pending_counts = {}    # (data_ptr, version) of num_tiles_hit -> (event, pinned view, keep-alive)


def _start_count(num_tiles_hit: Tensor, total: Optional[Tensor] = None, depth_parts=None) -> None:
    """total: the count already on its way (gg_project_fwd_count / gg_view_fwd left it there); None: count with a launch of
    its own.  depth_parts: (min bits, max bits, number of pairs) gg_view_fwd left behind, for gg_bin_sort_dev_ex"""
    dev = num_tiles_hit.device
    lib = _lib.load()
    ring, nxt = _pin_ring.get(dev.index, (None, 0))
    if ring is None:
        ring = torch.empty(_PIN_SLOTS, dtype=torch.int64).pin_memory()
    slot = ring[nxt:nxt + 1]
    _pin_ring[dev.index] = (ring, (nxt + 1) % _PIN_SLOTS)
    if total is None:
        total = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(lib.gg_count_intersects(num_tiles_hit.shape[0], _ptr(num_tiles_hit), _ptr(total), None, 0,
                                           _stream(dev)), "gg_count_intersects")
    slot.copy_(total, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    if len(_pending_counts) > 8:      # views whose count was never consumed
        _pending_counts.clear()
    _pending_counts[(num_tiles_hit.data_ptr(), num_tiles_hit._version)] = (ev, slot, num_tiles_hit, total, depth_parts)


def _pending(num_tiles_hit: Tensor):
    hit = _pending_counts.get((num_tiles_hit.data_ptr(), num_tiles_hit._version))
    if hit is None or hit[2] is not num_tiles_hit:
        return None
    return hit


def _take_count(num_tiles_hit: Tensor):
    hit = _pending(num_tiles_hit)
    if hit is None:
        return None
    _pending_counts.pop((num_tiles_hit.data_ptr(), num_tiles_hit._version), None)
    ev, slot = hit[0], hit[1]
    ev.synchronize()
    return int(slot.item())


# ------------------------------------------------------------------------------------------------
# ProjectGaussians
# ------------------------------------------------------------------------------------------------
class ProjectGaussians(Function):
    """gsplat.project_gaussians.ProjectGaussians.  apply(means3d, scales, glob_scale, quats,
    viewmat, projmat, fx, fy, cx, cy, img_height, img_width, tile_bounds, clip_thresh=0.01)
    -> (xys, depths, radii, conics, num_tiles_hit, cov3d)   [reference call :699-713]"""

    @staticmethod
    def forward(ctx, means3d: Tensor, scales: Tensor, glob_scale: float, quats: Tensor,
                viewmat: Tensor, projmat: Tensor, fx: float, fy: float, cx: float, cy: float,
                img_height: int, img_width: int, tile_bounds: Tuple[int, int, int],
                clip_thresh: float = CLIP_THRESH_DEFAULT):
        # cotangents nobody produced (cov3d always, others by route) arrive as None, not as zero-filled tensors:
        # autograd's default materialisation was a 24 MB fill kernel per view for cov3d alone
        ctx.set_materialize_grads(False)
        if means3d.ndim != 2 or means3d.shape[1] != 3:
            raise ValueError("means3d must have dimensions (N, 3)")
        n = means3d.shape[0]
        if tuple(scales.shape) != (n, 3):
            raise ValueError("scales must have dimensions (N, 3)")
        if tuple(quats.shape) != (n, 4):
            raise ValueError("quats must have dimensions (N, 4)")
        if viewmat.numel() < 12 or projmat.numel() != 16:
            raise ValueError("viewmat must hold >= 12 and projmat exactly 16 elements")
        dev = _require_hip(means3d, scales, quats, viewmat, projmat)
        ctx.sink = _sink_for(means3d, _dense_f32(means3d))
        means3d, scales, quats = _f32(means3d), _f32(scales), _f32(quats)
        viewmat, projmat = _f32(viewmat), _f32(projmat)
        lib = _lib.load()
        cov3d = torch.empty(n, 6, dtype=torch.float32, device=dev)
        xys = torch.empty(n, 2, dtype=torch.float32, device=dev)
        depths = torch.empty(n, dtype=torch.float32, device=dev)
        radii = torch.empty(n, dtype=torch.int32, device=dev)
        conics = torch.empty(n, 3, dtype=torch.float32, device=dev)
        num_tiles_hit = torch.empty(n, dtype=torch.int32, device=dev)
        # the projection also leaves sum(num_tiles_hit) on the device (one launch instead of projection + count + fill)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        cws = torch.empty(max(lib.gg_project_count_workspace(n) // 4, 1), dtype=torch.int32, device=dev)
        _lib.check(lib.gg_project_fwd_count(
            n, _ptr(means3d), _ptr(scales), float(glob_scale), _ptr(quats), _ptr(viewmat),
            _ptr(projmat), float(fx), float(fy), float(cx), float(cy), int(img_height),
            int(img_width), int(tile_bounds[0]), int(tile_bounds[1]), float(clip_thresh),
            _ptr(cov3d), _ptr(xys), _ptr(depths), _ptr(radii), _ptr(conics), _ptr(num_tiles_hit), _ptr(total),
            _ptr(cws), cws.numel() * 4, _stream(dev)), "gg_project_fwd_count")
        ctx.scalars = (float(glob_scale), float(fx), float(fy), float(cx), float(cy),
                       int(img_height), int(img_width))
        ctx.save_for_backward(means3d, scales, quats, viewmat, projmat, radii, conics)
        ctx.mark_non_differentiable(radii, num_tiles_hit)
        _start_count(num_tiles_hit, total)
        return xys, depths, radii, conics, num_tiles_hit, cov3d

    @staticmethod
    def backward(ctx, v_xys, v_depths, v_radii, v_conics, v_num_tiles_hit, v_cov3d):
        means3d, scales, quats, viewmat, projmat, radii, conics = ctx.saved_tensors
        glob_scale, fx, fy, cx, cy, img_height, img_width = ctx.scalars
        dev = means3d.device
        n = means3d.shape[0]
        # v_xys / v_conics usually are columns of the blend backward's interleaved record: read in place
        v_xys, xy_stride = _rows_or_zeros(v_xys, n, 2, dev)
        v_conics, conic_stride = _rows_or_zeros(v_conics, n, 3, dev)
        v_depths = torch.zeros(n, device=dev) if v_depths is None else _f32(v_depths)
        v_scale = torch.empty(n, 3, dtype=torch.float32, device=dev)
        v_quat = torch.empty(n, 4, dtype=torch.float32, device=dev)
        sink = ctx.sink
        v_mean3d = sink.buffer if sink is not None else torch.empty(n, 3, dtype=torch.float32, device=dev)
        lib = _lib.load()
        _lib.check(lib.gg_project_bwd_ex(
            n, _ptr(means3d), _ptr(scales), glob_scale, _ptr(quats), _ptr(viewmat), _ptr(projmat),
            fx, fy, cx, cy, img_height, img_width, _ptr(radii), _ptr(conics), _ptr(v_xys), xy_stride,
            _ptr(v_depths), _ptr(v_conics), conic_stride, _ptr(v_mean3d), 1 if sink is not None else 0,
            _ptr(v_scale), _ptr(v_quat), _stream(dev)), "gg_project_bwd_ex")
        if sink is not None:          # the means' gradient went straight into the registered buffer
            sink.done()
            v_mean3d = None
        return (v_mean3d, v_scale, None, v_quat, None, None, None, None, None, None, None, None,
                None, None)


# ------------------------------------------------------------------------------------------------
# SphericalHarmonics
# ------------------------------------------------------------------------------------------------
class SphericalHarmonics(Function):
    """gsplat.sh.SphericalHarmonics.  apply(degrees_to_use, viewdirs (N,3), coeffs (N,K,3))
    -> colors (N,3)   [reference call :730]"""

    @staticmethod
    def forward(ctx, degrees_to_use: int, viewdirs: Tensor, coeffs: Tensor):
        n, k = coeffs.shape[0], coeffs.shape[-2]
        assert k >= num_sh_bases(degrees_to_use), "not enough SH bases for degrees_to_use"
        deg_from_sh(k)  # raises ValueError on an invalid basis count
        if coeffs.shape[-1] != 3 or tuple(viewdirs.shape) != (n, 3):
            raise ValueError("viewdirs must be (N, 3) and coeffs (N, K, 3)")
        dev = _require_hip(viewdirs, coeffs)
        viewdirs, coeffs = _f32(viewdirs), _f32(coeffs)
        colors = torch.empty(n, 3, dtype=torch.float32, device=dev)
        lib = _lib.load()
        _lib.check(lib.gg_sh_fwd(n, k, int(degrees_to_use), _ptr(viewdirs), _ptr(coeffs),
                                 _ptr(colors), _stream(dev)), "gg_sh_fwd")
        ctx.degrees_to_use, ctx.num_bases = int(degrees_to_use), k
        ctx.save_for_backward(viewdirs)
        ctx.sink = _sink_for(coeffs, coeffs.dtype == torch.float32)
        return colors

    @staticmethod
    def backward(ctx, v_colors: Tensor):
        (viewdirs,) = ctx.saved_tensors
        dev, n = viewdirs.device, viewdirs.shape[0]
        v_colors = _f32(v_colors)
        lib = _lib.load()
        sink = ctx.sink
        if sink is not None:          # add into the registered gradient buffer, hand autograd nothing
            if sink.keeps_sh():       # expand the step's views in one pass (see ShadeTail)
                sink.keep_sh(ctx.degrees_to_use, ctx.num_bases, viewdirs, v_colors)
                return None, None, None
            _lib.check(lib.gg_sh_bwd_accumulate(n, ctx.num_bases, ctx.degrees_to_use, _ptr(viewdirs),
                                                _ptr(v_colors), _ptr(sink.buffer), _stream(dev)),
                       "gg_sh_bwd_accumulate")
            sink.done()
            return None, None, None
        v_coeffs = torch.empty(n, ctx.num_bases, 3, dtype=torch.float32, device=dev)
        _lib.check(lib.gg_sh_bwd(n, ctx.num_bases, ctx.degrees_to_use, _ptr(viewdirs),
                                 _ptr(v_colors), _ptr(v_coeffs), _stream(dev)), "gg_sh_bwd")
        return None, None, v_coeffs


def _rows_in_place(t: Tensor, width: int):
    """(tensor, row stride in floats) for a (N, width) fp32 cotangent whose rows can be read where they are — a
    dense array or the columns of a wider record (the blend backward's interleaved gradient record); anything
    else is copied to a dense array first."""
    if t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == width and t.stride(1) == 1 \
            and t.stride(0) >= width and t.data_ptr() % 4 == 0:
        return t, t.stride(0)
    t = _f32(t).reshape(-1, width)
    return t, width


def _rows_or_zeros(v: Optional[Tensor], n: int, width: int, dev: torch.device):
    """_rows_in_place of a (N, width) cotangent; zeros for one that nobody produced (None)."""
    return (torch.zeros(n, width, device=dev), width) if v is None else _rows_in_place(v, width)


class ShadeTail(Function):
    """apply(degrees_to_use, viewdirs (N,3), coeffs (N,K,3), depths (N,), normals (N,3)) -> tail (N, 7) =
    [ clamp(SphericalHarmonics(...) + 0.5, 0, 1) | depth | normal ]: the 7-channel colour array of the plugin
    route's rasterize operator in one kernel each way (reference :730-731 clamp, :765 depth, :779 normal colours).
    The backward reads the cotangent rows in place (the blend backward's interleaved gradient record, any row
    stride) and adds the SH gradient into a registered gradient sink like SphericalHarmonics does.

    one_wave (optional sixth argument): launch the forward in one-wave workgroups (gg_shade_tail_fwd_ex: the same bits).
    For a forward that runs beside a blend kernel of another stream — forward(k + 1) beside backward(k) in
    dist.train_step_pipelined: the blend kernels refill every slot they free, so the default 256-thread workgroups with
    38 KB of LDS are not placed until the backward drains (620 us instead of 65) and binning and the pair forward wait
    behind them; one-wave workgroups are placed slot by slot (profiles/forward_chain_overlap.txt).  Alone on the GPU the
    default launch is no slower."""

    @staticmethod
    def forward(ctx, degrees_to_use: int, viewdirs: Tensor, coeffs: Tensor, depths: Tensor, normals: Tensor,
                one_wave: bool = False):
        n, k = coeffs.shape[0], coeffs.shape[-2]
        assert k >= num_sh_bases(degrees_to_use), "not enough SH bases for degrees_to_use"
        deg_from_sh(k)
        if coeffs.shape[-1] != 3 or tuple(viewdirs.shape) != (n, 3):
            raise ValueError("viewdirs must be (N, 3) and coeffs (N, K, 3)")
        if tuple(depths.shape) != (n,) or tuple(normals.shape) != (n, 3):
            raise ValueError("depths must be (N,) and normals (N, 3)")
        dev = _require_hip(viewdirs, coeffs, depths, normals)
        viewdirs, coeffs, depths_c, normals_c = _f32(viewdirs), _f32(coeffs), _f32(depths), _f32(normals)
        tail = torch.empty(n, 7, dtype=torch.float32, device=dev)
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        if one_wave:
            _lib.check(_lib.load().gg_shade_tail_fwd_ex(n, k, int(degrees_to_use), _ptr(viewdirs), _ptr(coeffs),
                                                        _ptr(depths_c), _ptr(normals_c), _ptr(tail), _ptr(mask), 1,
                                                        _stream(dev)), "gg_shade_tail_fwd_ex")
        else:
            _lib.check(_lib.load().gg_shade_tail_fwd(n, k, int(degrees_to_use), _ptr(viewdirs), _ptr(coeffs),
                                                     _ptr(depths_c), _ptr(normals_c), _ptr(tail), _ptr(mask),
                                                     _stream(dev)), "gg_shade_tail_fwd")
        ctx.degrees_to_use, ctx.num_bases = int(degrees_to_use), k
        ctx.save_for_backward(viewdirs, mask)
        ctx.sink = _sink_for(coeffs, coeffs.dtype == torch.float32)
        return tail

    @staticmethod
    def backward(ctx, v_tail: Tensor):
        viewdirs, mask = ctx.saved_tensors
        dev, n = viewdirs.device, viewdirs.shape[0]
        v_tail, stride = _rows_in_place(v_tail, 7)
        v_depths = torch.empty(n, dtype=torch.float32, device=dev)
        v_normals = torch.empty(n, 3, dtype=torch.float32, device=dev)
        lib = _lib.load()
        sink = ctx.sink
        if sink is not None and sink.keeps_sh():
            # keep this view's SH gradient as its factors; all kept views are expanded once (the last view of the
            # step, or flush_grad_sinks())
            v_rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
            _lib.check(lib.gg_shade_tail_bwd_split(n, _ptr(v_tail), stride, _ptr(mask), _ptr(v_rgb),
                                                   _ptr(v_depths), _ptr(v_normals), _stream(dev)),
                       "gg_shade_tail_bwd_split")
            sink.keep_sh(ctx.degrees_to_use, ctx.num_bases, viewdirs, v_rgb)
            return None, None, None, v_depths, v_normals, None
        v_coeffs = sink.buffer if sink is not None \
            else torch.empty(n, ctx.num_bases, 3, dtype=torch.float32, device=dev)
        _lib.check(lib.gg_shade_tail_bwd(n, ctx.num_bases, ctx.degrees_to_use, _ptr(viewdirs), _ptr(v_tail), stride,
                                         _ptr(mask), _ptr(v_coeffs), 1 if sink is not None else 0, _ptr(v_depths),
                                         _ptr(v_normals), _stream(dev)), "gg_shade_tail_bwd")
        if sink is not None:
            sink.done()
            v_coeffs = None
        return None, None, v_coeffs, v_depths, v_normals, None


# ------------------------------------------------------------------------------------------------
# binning shared by the rasterize calls of one view
# ------------------------------------------------------------------------------------------------
class Binning:
    """Result of compute_cumulative_intersects + bin_and_sort_gaussians for one view.

    `num_intersects` may still be unknown to the host when the lists are already being built on the
    device (speculative capacity, below): `resolve()` waits for the asynchronous read-back of the
    count — by then the sort and the first blend kernel are queued behind it, so the GPU does not idle —
    and re-bins with an exact size in the rare case the capacity was too small."""
    __slots__ = ("num_intersects", "gaussian_ids_sorted", "tile_bins", "key", "keep", "_redo")

    def __init__(self, num_intersects, gaussian_ids_sorted, tile_bins, key, keep, redo=None):
        self.num_intersects = num_intersects
        self.gaussian_ids_sorted = gaussian_ids_sorted
        self.tile_bins = tile_bins
        self.key = key
        self.keep = keep  # the keyed tensors stay alive so data_ptr cannot be recycled
        self._redo = redo

    def resolve(self) -> bool:
        """Make `num_intersects` known.  Returns True if the lists had to be rebuilt (whatever was
        rendered from them must be rendered again)."""
        if self.num_intersects is not None:
            return False
        return self._redo(self)


_bin_cache: Optional[Binning] = None
bin_cache_stats = {"hits": 0, "misses": 0, "speculative": 0, "rebinned": 0}
_capacity_hint = {}     # device index -> list capacity that covered the views seen so far


def _bin_key(xys, depths, radii, num_tiles_hit, img_height, img_width):
    return tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in
                 (xys, depths, radii, num_tiles_hit)) + (int(img_height), int(img_width))


def last_num_intersects(radii: Optional[Tensor] = None) -> Optional[int]:
    """Length of the tile lists of the view binned last, once known to the host (the rasterize operators resolve
    it before they return); None before any binning.  0 means nothing was visible — what the reference's
    `(self.radii).sum() == 0` (gaussian_splatting.py:714) asks with a host round trip BEFORE the render.
    With `radii` (the projection output of THIS call): None as well unless the lists binned last are this call's —
    a view whose operator did not bin must not be judged by the previous view's count."""
    if _bin_cache is None:
        return None
    if radii is not None and not any(t is radii for t in _bin_cache.keep):
        return None
    return _bin_cache.num_intersects


def clear_bin_cache() -> None:
    global _bin_cache
    _bin_cache = None


def _note_count(dev: torch.device, num_intersects: int) -> None:
    want = ((int(num_intersects * 1.25) >> 20) + 1) << 20        # 25 % headroom, whole Mi entries
    if want > _capacity_hint.get(dev.index, 0):
        _capacity_hint[dev.index] = want


def bin_and_sort_gaussians(xys: Tensor, depths: Tensor, radii: Tensor, num_tiles_hit: Tensor,
                           img_height: int, img_width: int, use_cache: bool = True,
                           speculative: bool = False) -> Binning:
    """Tile lists of one view: Gaussian ids tile-major / near-to-far, and per-tile [start,end).

    The reference reads the intersection count with `.item()` before it can size and launch the sort
    (SURVEY a5): the GPU drains while the host waits, then idles while the host enqueues.  Here, once a
    view has been seen, the lists are built with a capacity that covered the previous views (+25 %) and
    the kernels take the actual count from device memory (gg_bin_sort_dev); the count is read back
    asynchronously and only checked later (`Binning.resolve`).  `speculative=False` (the default for
    direct callers) returns with `num_intersects` known."""
    global _bin_cache
    dev = _require_hip(xys, depths, radii, num_tiles_hit)
    key = _bin_key(xys, depths, radii, num_tiles_hit, img_height, img_width)
    if use_cache and _bin_cache is not None and _bin_cache.key == key:
        bin_cache_stats["hits"] += 1
        if not speculative:
            _bin_cache.resolve()
        return _bin_cache
    bin_cache_stats["misses"] += 1
    lib = _lib.load()
    n = xys.shape[0]
    tiles_x = (img_width + BLOCK - 1) // BLOCK
    tiles_y = (img_height + BLOCK - 1) // BLOCK
    xys_c, depths_c = _f32(xys.detach()), _f32(depths.detach())
    radii_c, nth_c = _i32(radii), _i32(num_tiles_hit)
    tile_bins = torch.empty(tiles_x * tiles_y, 2, dtype=torch.int32, device=dev)
    keep = (xys, depths, radii, num_tiles_hit)

    def exact(num_intersects: int) -> Tensor:
        ids = torch.empty(max(num_intersects, 1), dtype=torch.int32, device=dev)
        ws = _workspace(lib.gg_bin_sort_workspace(n, num_intersects), dev)
        _lib.check(lib.gg_bin_sort(n, num_intersects, _ptr(xys_c), _ptr(depths_c), _ptr(radii_c),
                                   _ptr(nth_c), tiles_x, tiles_y, _ptr(ids), _ptr(tile_bins),
                                   None, _ptr(ws), ws.numel(), _stream(dev)), "gg_bin_sort")
        return ids[:num_intersects]

    pending = _pending(num_tiles_hit) if speculative else None
    cap = _capacity_hint.get(dev.index, 0)
    if pending is not None and cap > 0:
        # speculative: sized by what previous views needed, count taken on the device
        bin_cache_stats["speculative"] += 1
        total_dev = pending[3]
        ids = torch.empty(cap, dtype=torch.int32, device=dev)
        ws = _workspace(lib.gg_bin_sort_workspace(n, cap), dev)
        parts = pending[4]                # (min bits, max bits, pairs) from the projection, or None
        _lib.check(lib.gg_bin_sort_dev_ex(n, cap, _ptr(total_dev), _ptr(xys_c), _ptr(depths_c), _ptr(radii_c),
                                          _ptr(nth_c), tiles_x, tiles_y, _ptr(ids), _ptr(tile_bins),
                                          None, _ptr(ws), ws.numel(), _ptr(parts[0]) if parts else None,
                                          _ptr(parts[1]) if parts else None, parts[2] if parts else 0, _stream(dev)),
                   "gg_bin_sort_dev_ex")

        def redo(b: Binning) -> bool:
            count = _take_count(num_tiles_hit)
            if count is None:                              # read-back already consumed by another binning
                count = int(total_dev.item())
            _note_count(dev, count)
            b.num_intersects = count
            if count <= cap:
                b.gaussian_ids_sorted = ids[:count]
                return False
            bin_cache_stats["rebinned"] += 1
            b.gaussian_ids_sorted = exact(count)
            return True

        out = Binning(None, ids, tile_bins, key, keep, redo)
    else:
        num_intersects = _take_count(num_tiles_hit)       # started by ProjectGaussians.forward
        if num_intersects is None:                        # tensors that did not come from our projection
            total = torch.empty(1, dtype=torch.int64, device=dev)
            _lib.check(lib.gg_count_intersects(n, _ptr(nth_c), _ptr(total), None, 0, _stream(dev)),
                       "gg_count_intersects")
            num_intersects = int(total.item())
        _note_count(dev, num_intersects)
        out = Binning(num_intersects, exact(num_intersects), tile_bins, key, keep)
    if use_cache:
        _bin_cache = out
    return out


# ------------------------------------------------------------------------------------------------
# Rasterize
# ------------------------------------------------------------------------------------------------
def _blend_with_lists(bins: Binning, launch) -> bool:
    """Enqueue the forward blend (`launch()` reads bins.gaussian_ids_sorted / tile_bins when called), then make the
    lists' length known: a speculative binning's count is checked only with the blend already queued, and rebuilt
    lists (capacity too small: rare) mean blending once more.  False: nothing is visible, there is no image."""
    for attempt in range(2):
        if bins.num_intersects is not None and bins.num_intersects < 1:
            return False
        launch()
        if not bins.resolve():
            break
    return bins.num_intersects >= 1


@torch.no_grad()
def blend_votes(xys: Tensor, depths: Tensor, radii: Tensor, conics: Tensor, num_tiles_hit: Tensor, opacity: Tensor,
                img_height: int, img_width: int, labels: Tensor, votes: Tensor) -> bool:
    """The transpose of the blend (`gg_blend_votes`): votes[g, l] += sum over the pixels of label l of
    trunc(alpha T 2^24), alpha T being the weight with which the exact forward walk blends Gaussian g there.
    labels (H, W) uint8, a label >= votes.shape[1] (255: ignore) votes for nobody; votes (N, L) int64, contiguous,
    ADDED to.  The lists are those of a render of the same view (one binning, cached).  False: nothing is visible,
    votes is untouched."""
    if xys.ndimension() != 2 or xys.size(1) != 2:
        raise ValueError("xys must have dimensions (N, 2)")
    n = xys.size(0)
    img_height, img_width = int(img_height), int(img_width)
    if labels.dtype != torch.uint8 or tuple(labels.shape) != (img_height, img_width):
        raise ValueError(f"labels must be a uint8 ({img_height}, {img_width}) tensor, got {labels.dtype} "
                         f"{tuple(labels.shape)}")
    if votes.dtype != torch.int64 or votes.ndimension() != 2 or votes.size(0) != n or not votes.is_contiguous():
        raise ValueError(f"votes must be a contiguous int64 ({n}, L) tensor, got {votes.dtype} {tuple(votes.shape)}")
    num_labels = votes.size(1)
    if not 1 <= num_labels <= 255:
        raise ValueError(f"votes must have 1..255 label columns, got {num_labels}")
    if opacity.numel() != n:
        raise ValueError(f"opacity must have {n} entries, got {tuple(opacity.shape)}")
    dev = _require_hip(xys, depths, radii, conics, num_tiles_hit, opacity, labels, votes)
    if n == 0:
        return False
    xys_c, conics_c, opacity_c = _f32(xys.detach()), _f32(conics.detach()), _f32(opacity.detach())
    labels_c = labels.contiguous()
    bins = bin_and_sort_gaussians(xys, depths, radii, num_tiles_hit, img_height, img_width, speculative=True)
    lib = _lib.load()
    ws = _workspace(lib.gg_blend_workspace(n), dev)
    # The call adds, so a walk over lists that turn out truncated (speculative capacity too small: rare) must not
    # reach `votes`: while the lists' length is unknown the walk adds to a zeroed scratch array instead, which is
    # added to `votes` once the lists are known to be whole (integer adds: the same bits either way).
    scratch = []

    def launch():
        out = votes
        if bins.num_intersects is None:
            out = torch.zeros_like(votes)
            scratch[:] = [out]
        else:
            scratch.clear()
        _lib.check(lib.gg_blend_votes(num_labels, n, img_height, img_width, _ptr(bins.gaussian_ids_sorted),
                                      _ptr(bins.tile_bins), _ptr(xys_c), _ptr(conics_c), _ptr(opacity_c),
                                      _ptr(labels_c), _ptr(out), _ptr(ws), ws.numel(), 0, _stream(dev)),
                   "gg_blend_votes")

    if not _blend_with_lists(bins, launch):
        return False
    if scratch:
        votes.add_(scratch[0])
    return True


def check_t_hit(t_hit: float) -> float:
    """t_hit as gg_blend_hits takes it: a float32 strictly between GG_T_EPS (1e-4) and 1."""
    t = C.c_float(float(t_hit)).value
    if not C.c_float(1e-4).value < t < 1.0:                      # NaN fails
        raise ValueError(f"t_hit must be in (1e-4, 1), got {t_hit}")
    return t


@torch.no_grad()
def blend_hits(xys: Tensor, depths: Tensor, radii: Tensor, conics: Tensor, num_tiles_hit: Tensor, opacity: Tensor,
               img_height: int, img_width: int, t_hit: float = 0.5, full: bool = True):
    """What the exact forward walk finds under every pixel (`gg_blend_hits`): (hit_idx, top_idx, top_vis, count),
    each (H, W).  hit_idx int32: the Gaussian at which the transmittance falls to <= t_hit (the median Gaussian for
    0.5), -1 where it never does; top_idx int32 / top_vis float32: the Gaussian with the largest blend weight alpha T
    and that weight (-1 / 0: nothing blended); count int32: the number of blended Gaussians.  full=False returns
    (hit_idx, None, None, None) from a walk that leaves every pixel at its hit.  The lists are those of a render of
    the same view (one binning, cached).  Nothing visible: the defaults everywhere."""
    if xys.ndimension() != 2 or xys.size(1) != 2:
        raise ValueError("xys must have dimensions (N, 2)")
    n = xys.size(0)
    img_height, img_width = int(img_height), int(img_width)
    if img_height < 1 or img_width < 1:
        raise ValueError(f"the image must have at least one pixel, got ({img_height}, {img_width})")
    t_hit = check_t_hit(t_hit)
    if conics.ndimension() != 2 or tuple(conics.shape) != (n, 3):
        raise ValueError(f"conics must have dimensions ({n}, 3), got {tuple(conics.shape)}")
    if opacity.numel() != n:
        raise ValueError(f"opacity must have {n} entries, got {tuple(opacity.shape)}")
    dev = _require_hip(xys, depths, radii, conics, num_tiles_hit, opacity)
    shape = (img_height, img_width)
    hit_idx = torch.empty(shape, dtype=torch.int32, device=dev)
    outs = [hit_idx, None, None, None]
    if full:
        outs[1:] = [torch.empty(shape, dtype=torch.int32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev),
                    torch.empty(shape, dtype=torch.int32, device=dev)]

    def defaults():
        hit_idx.fill_(-1)
        if full:
            outs[1].fill_(-1)
            outs[2].zero_()
            outs[3].zero_()
        return tuple(outs)

    if n == 0:
        return defaults()
    xys_c, conics_c, opacity_c = _f32(xys.detach()), _f32(conics.detach()), _f32(opacity.detach())
    bins = bin_and_sort_gaussians(xys, depths, radii, num_tiles_hit, img_height, img_width, speculative=True)
    lib = _lib.load()
    ws = _workspace(lib.gg_blend_workspace(n), dev)

    # the call overwrites every pixel, so a walk over lists that turn out truncated is simply walked again
    def launch():
        _lib.check(lib.gg_blend_hits(n, img_height, img_width, _ptr(bins.gaussian_ids_sorted), _ptr(bins.tile_bins),
                                     _ptr(xys_c), _ptr(conics_c), _ptr(opacity_c), t_hit, *(_ptr(t) for t in outs),
                                     _ptr(ws), ws.numel(), 0, _stream(dev)), "gg_blend_hits")

    if not _blend_with_lists(bins, launch):
        return defaults()
    return tuple(outs)


def _rasterize_forward(ctx, xys, depths, radii, conics, num_tiles_hit, colors, opacity,
                       img_height, img_width, background, three_channel_only):
    if colors.dtype == torch.uint8:
        colors = colors.float() / 255
    if background is not None:
        assert background.shape[0] == colors.shape[-1], \
            f"incorrect shape of background color tensor, expected shape {colors.shape[-1]}"
    else:
        background = torch.ones(colors.shape[-1], dtype=torch.float32, device=colors.device)
    if xys.ndimension() != 2 or xys.size(1) != 2:
        raise ValueError("xys must have dimensions (N, 2)")
    if three_channel_only:
        if colors.ndimension() != 2 or colors.size(1) != 3:
            raise ValueError("colors must have dimensions (N, 3)")
    elif colors.ndimension() != 2:
        raise ValueError("colors must have dimensions (N, D)")
    if opacity.ndimension() != 2 or opacity.size(1) != 1:
        raise ValueError("opacity must have dimensions (N, 1)")
    dev = _require_hip(xys, depths, radii, conics, num_tiles_hit, colors, opacity, background)
    n, ch = xys.size(0), colors.size(1)
    # wide colour gradients can go straight into a registered buffer (32-channel rows stay dense)
    ctx.sink = _sink_for(colors, ch > 3 and _dense_f32(colors))
    img_height, img_width = int(img_height), int(img_width)
    xys_c, conics_c = _f32(xys), _f32(conics)
    colors_c, opacity_c, background = _f32(colors), _f32(opacity), _f32(background)

    bins = bin_and_sort_gaussians(xys, depths, radii, num_tiles_hit, img_height, img_width, speculative=True)
    ctx.img = (img_height, img_width)
    ctx.opacity_shape = tuple(opacity.shape)
    lib = _lib.load()
    ws = _workspace(lib.gg_blend_workspace(n), dev)
    out_img = torch.empty(img_height, img_width, ch, dtype=torch.float32, device=dev)
    final_Ts = torch.empty(img_height, img_width, dtype=torch.float32, device=dev)
    final_idx = torch.empty(img_height, img_width, dtype=torch.int32, device=dev)

    def launch():
        _lib.check(lib.gg_blend_fwd(ch, n, img_height, img_width, _ptr(bins.gaussian_ids_sorted),
                                    _ptr(bins.tile_bins), _ptr(xys_c), _ptr(conics_c), _ptr(colors_c),
                                    _ptr(opacity_c), _ptr(background), _ptr(out_img), _ptr(final_Ts),
                                    _ptr(final_idx), _ptr(ws), ws.numel(), _stream(dev)), "gg_blend_fwd")

    visible = _blend_with_lists(bins, launch)
    ctx.num_intersects = bins.num_intersects
    if not visible:
        ctx.save_for_backward(xys_c, conics_c, colors_c, opacity_c)
        return torch.ones(img_height, img_width, ch, device=dev) * background
    # ws holds the packed per-Gaussian records of this call: the backward reuses them
    ctx.save_for_backward(xys_c, conics_c, colors_c, opacity_c, background,
                          bins.gaussian_ids_sorted, bins.tile_bins, final_Ts, final_idx, ws)
    return out_img


_DETERMINISTIC = False
# True: the fused operator's forward walk (feature 32 | rgb + depth + normal) runs the exact-summation-order kernel —
# images bit-identical to the oracle's sequential fma chain (gg_blend_fwd_pair); False (default): the batched kernel with
# fp16 two-piece products (gg_blend_fwd_pair_fast): same final_T / final_idx / decisions, images to fp32 rounding
# (~1e-7 of the colours' range; BASELINE asks for 1e-5).  Like mlp.EXACT_ORDER.
EXACT_FORWARD = False


def set_exact_forward(on: bool = True) -> bool:
    global EXACT_FORWARD
    prev, EXACT_FORWARD = EXACT_FORWARD, bool(on)
    return prev


def set_fast_forward(on: bool = True) -> bool:
    return not set_exact_forward(not on)


def set_deterministic_backward(on: bool = True) -> bool:
    """Bit-reproducible blend gradients.  The default backward adds pixel contributions with float atomics,
    whose order changes from run to run (as in gsplat 0.1.0: csrc/backward.cu atomicAdd).  With this switch the
    kernels store the total of every (tile-list entry, quadrant) instead and a second pass sums each
    Gaussian's entries in list order (`gg_blend_bwd_deterministic`): same values to ~1 ulp of the largest term,
    identical bits on every run, at the price of 16 (C + 6) bytes of scratch per list entry and roughly twice
    the time.  Returns the previous setting."""
    global _DETERMINISTIC
    prev, _DETERMINISTIC = _DETERMINISTIC, bool(on)
    return prev


def _blend_bwd(lib, ch, n, img_height, img_width, ids_sorted, tile_bins, xys, conics, colors, opacity, background,
               final_Ts, final_idx, v_out, v_xy, v_conic, v_colors, v_opacity, gstride, cstride, ws, flags,
               num_intersects):
    dev = xys.device
    if not _DETERMINISTIC:
        _lib.check(lib.gg_blend_bwd(ch, n, img_height, img_width, _ptr(ids_sorted), _ptr(tile_bins), _ptr(xys),
                                    _ptr(conics), _ptr(colors), _ptr(opacity), _ptr(background), _ptr(final_Ts),
                                    _ptr(final_idx), _ptr(v_out), _ptr(v_xy), _ptr(v_conic), _ptr(v_colors),
                                    _ptr(v_opacity), gstride, cstride, _ptr(ws), ws.numel(), flags,
                                    _stream(dev)), "gg_blend_bwd")
        return
    det_ws = _workspace(lib.gg_blend_bwd_deterministic_workspace(n, ch, num_intersects), dev)
    _lib.check(lib.gg_blend_bwd_deterministic(ch, n, img_height, img_width, _ptr(ids_sorted), _ptr(tile_bins),
                                              _ptr(xys), _ptr(conics), _ptr(colors), _ptr(opacity),
                                              _ptr(background), _ptr(final_Ts), _ptr(final_idx), _ptr(v_out),
                                              _ptr(v_xy), _ptr(v_conic), _ptr(v_colors), _ptr(v_opacity), gstride,
                                              cstride, _ptr(ws), ws.numel(), flags, num_intersects, _ptr(det_ws),
                                              det_ws.numel(), _stream(dev)), "gg_blend_bwd_deterministic")


def _rasterize_backward(ctx, v_out_img):
    img_height, img_width = ctx.img
    if ctx.num_intersects < 1:
        xys, conics, colors, opacity = ctx.saved_tensors
        v_xy, v_conic = torch.zeros_like(xys), torch.zeros_like(conics)
        v_colors, v_opacity = torch.zeros_like(colors), torch.zeros_like(opacity)
    else:
        (xys, conics, colors, opacity, background, ids_sorted, tile_bins, final_Ts,
         final_idx, ws) = ctx.saved_tensors
        dev, n, ch = xys.device, xys.shape[0], colors.shape[1]
        v_out_img = _f32(v_out_img)
        # Gradient layout: the kernels add with float atomics, and what they cost is cache lines
        # touched per instruction — so the geometry gradients of a Gaussian sit in ONE interleaved
        # record {xy, conic, opacity} (+ the colours for <= 3 channels); the tensors handed back to
        # autograd are strided views of it.  32-channel colour rows stay dense (128-byte rows).
        # (records padded to 64 / 32 bytes so that none straddles a line measure the same.)
        flags = 1                      # ws holds the forward's packed records
        sink = getattr(ctx, "sink", None)
        if ch <= 3:
            rec_g = torch.empty(n, 6 + ch, dtype=torch.float32, device=dev)
            v_colors = rec_g[:, 6:]
            gstride = cstride = 6 + ch
        else:
            rec_g = torch.empty(n, 6, dtype=torch.float32, device=dev)
            if sink is not None:       # atomics add into the caller's gradient buffer: no memset, no add
                v_colors = sink.buffer
                flags |= 2
            else:
                v_colors = torch.empty(n, ch, dtype=torch.float32, device=dev)   # own allocation: aligned rows
            gstride, cstride = 6, 0
        v_xy, v_conic, v_opacity = rec_g[:, 0:2], rec_g[:, 2:5], rec_g[:, 5:6]
        lib = _lib.load()
        _blend_bwd(lib, ch, n, img_height, img_width, ids_sorted, tile_bins, xys, conics, colors, opacity,
                   background, final_Ts, final_idx, v_out_img, v_xy, v_conic, v_colors, v_opacity, gstride,
                   cstride, ws, flags, ctx.num_intersects)
        if flags & 2:
            v_colors = None
            sink.done()
    return (v_xy, None, None, v_conic, None, v_colors, v_opacity.reshape(ctx.opacity_shape),
            None, None, None)


class RasterizeGaussians(Function):
    """gsplat.rasterize.RasterizeGaussians (3 colour channels).  apply(xys, depths, radii, conics,
    num_tiles_hit, colors (N,3), opacity (N,1), img_height, img_width, background=None)
    -> out_img (H,W,3)   [reference calls :735-746 rgb, :759-770 depth, :773-784 normal]"""

    @staticmethod
    def forward(ctx, xys, depths, radii, conics, num_tiles_hit, colors, opacity, img_height,
                img_width, background=None):
        return _rasterize_forward(ctx, xys, depths, radii, conics, num_tiles_hit, colors, opacity,
                                  img_height, img_width, background, True)

    backward = staticmethod(_rasterize_backward)


class NDRasterizeGaussians(Function):
    """gsplat.nd_rasterize.NDRasterizeGaussians (any channel count).  Same signature with
    colors (N,D) -> out_img (H,W,D)   [reference call :747-758, D = 32 feature channels]"""

    @staticmethod
    def forward(ctx, xys, depths, radii, conics, num_tiles_hit, colors, opacity, img_height,
                img_width, background=None):
        return _rasterize_forward(ctx, xys, depths, radii, conics, num_tiles_hit, colors, opacity,
                                  img_height, img_width, background, False)

    backward = staticmethod(_rasterize_backward)


# ------------------------------------------------------------------------------------------------
# caller-side activations of a view in one kernel each way
# ------------------------------------------------------------------------------------------------
class ActivateGaussians(Function):
    """apply(means, log_scales, quats, opacities (N,1) logits, cam_pos (3,)) ->
    (scales (N,3), quats_n (N,4), opac (N,1), viewdirs (N,3), normals (N,3)): the reference's
    `torch.exp(scales)` (:701), `quats / quats.norm(dim=-1, keepdim=True)` (:703),
    `torch.sigmoid(opacities)` (:742), view directions (:727-728, no gradient) and `get_normals()`
    (:605-619) — ~12 torch launches forward and ~25 backward per view in the reference, one launch each
    way here.  Used by the plugin's fused model; the shim route leaves the caller's torch ops alone."""

    @staticmethod
    def forward(ctx, means, log_scales, quats, opacities, cam_pos):
        ctx.set_materialize_grads(False)   # undefined cotangents arrive as None (handled in backward)
        dev = _require_hip(means, log_scales, quats, opacities, cam_pos)
        n = means.shape[0]
        if tuple(log_scales.shape) != (n, 3) or tuple(quats.shape) != (n, 4) or opacities.numel() != n:
            raise ValueError("expected means (N,3), scales (N,3), quats (N,4), opacities (N,1)")
        m, s, q, o, c = _f32(means), _f32(log_scales), _f32(quats), _f32(opacities), _f32(cam_pos).reshape(-1)
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        scales, quats_n, opac, viewdirs, normals = f(n, 3), f(n, 4), f(n, 1), f(n, 3), f(n, 3)
        axis = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().gg_activate_fwd(n, _ptr(m), _ptr(s), _ptr(q), _ptr(o), _ptr(c), _ptr(scales),
                                               _ptr(quats_n), _ptr(opac), _ptr(viewdirs), _ptr(normals), _ptr(axis),
                                               _stream(dev)), "gg_activate_fwd")
        ctx.save_for_backward(q, scales, opac, axis)
        ctx.opacity_shape = tuple(opacities.shape)
        ctx.sinks = _sinks_for_all(log_scales, quats, opacities)
        ctx.mark_non_differentiable(viewdirs)
        return scales, quats_n, opac.reshape(ctx.opacity_shape), viewdirs, normals

    @staticmethod
    def backward(ctx, v_scales, v_quats_n, v_opac, v_viewdirs, v_normals):
        q, scales, opac, axis = ctx.saved_tensors
        dev, n = q.device, q.shape[0]
        z = lambda t, *shape: torch.zeros(*shape, dtype=torch.float32, device=dev) if t is None else _f32(t)
        v_scales, v_quats_n = z(v_scales, n, 3), z(v_quats_n, n, 4)
        v_normals = z(v_normals, n, 3)
        # v_opac usually is column 5 of the blend backward's interleaved record: read in place
        v_opac, opac_stride = (torch.zeros(n, 1, device=dev), 1) if v_opac is None \
            else _rows_in_place(v_opac.reshape(n, 1), 1)
        e = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        # with sinks: add straight into the registered gradient buffers
        v_ls, v_q, v_o = (k.buffer for k in ctx.sinks) if ctx.sinks is not None else (e(n, 3), e(n, 4), e(n, 1))
        _lib.check(_lib.load().gg_activate_bwd_ex(
            n, _ptr(q), _ptr(scales), _ptr(opac), _ptr(axis), _ptr(v_scales), _ptr(v_quats_n), _ptr(v_opac),
            opac_stride, _ptr(v_normals), _ptr(v_ls), _ptr(v_q), _ptr(v_o), 1 if ctx.sinks is not None else 0,
            _stream(dev)), "gg_activate_bwd_ex")
        if ctx.sinks is not None:
            for sink in ctx.sinks:
                sink.done()
            return None, None, None, None, None
        return None, v_ls, v_q, v_o.reshape(ctx.opacity_shape), None


# ------------------------------------------------------------------------------------------------
# the per-Gaussian chain of a view as ONE autograd node (round 4; what the plugin's fused model calls)
# ------------------------------------------------------------------------------------------------
class _PartCtx:
    """The `ctx` of a Function whose forward / backward run INSIDE another Function (ViewGeometry): attributes are kept,
    saved tensors are handed to the outer ctx.save_for_backward (a tensor held as a plain attribute of a node that
    produced it would be a reference cycle)."""

    def __init__(self):
        self.saved_tensors = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        pass

    def set_materialize_grads(self, value):
        pass


def _pose_outputs(lib, n: int, dev: torch.device):
    """(v_viewmat (12,), v_full_proj (16,), workspace) of the kernels that sum the camera's gradient"""
    return (torch.empty(12, dtype=torch.float32, device=dev), torch.empty(16, dtype=torch.float32, device=dev),
            _workspace(lib.gg_pose_grad_workspace(n), dev))


def _is_record_view(t: Optional[Tensor], base: int, offset: int, width: int, stride: int, n: int) -> bool:
    return (t is not None and t.dtype == torch.float32 and t.dim() == 2 and tuple(t.shape) == (n, width)
            and t.stride(1) == 1 and t.stride(0) == stride and t.data_ptr() == base + 4 * offset)


class ViewGeometry(Function):
    """apply(means, log_scales, quats, opacities, colors_all, cam_pos, viewmat, full_proj, fx, fy, cx, cy,
             img_height, img_width, tile_bounds, degrees_to_use[, one_wave_sh = False: ShadeTail's `one_wave`])
       -> (xys, depths, radii, conics, num_tiles_hit, opac, tail (N, 7), normals, packed)

    `packed`: a blend workspace already holding these Gaussians' packed records (pass it to rasterize_segments(...,
    packed=...): the forward then skips its packing pass).

    ActivateGaussians -> ProjectGaussians -> ShadeTail (reference :699-731, :742, :605-619) as one node: the forward is
    those three operators' forwards, the backward — when every parameter has a gradient buffer (register_grad_sink) and
    the cotangents arrive as the columns of the blend backward's per-Gaussian record, i.e. in the plugin's training
    step — is ONE kernel (gg_view_bwd) instead of three that hand (N, k) arrays to each other; the SH gradient is kept
    or expanded exactly as ShadeTail does.  Anything else (no sinks, dense cotangents, extra cotangents for depths /
    normals) runs the three operators' backwards in order: same values either way (shared device code)."""

    @staticmethod
    def forward(ctx, means, log_scales, quats, opacities, colors_all, cam_pos, viewmat, full_proj, fx, fy, cx, cy,
                img_height, img_width, tile_bounds, degrees_to_use, one_wave_sh=False):
        ctx.set_materialize_grads(False)
        a, p, t = _PartCtx(), _PartCtx(), _PartCtx()
        scales_e, quats_n, opac, viewdirs, normals, xys, depths, radii, conics, num_tiles_hit, packed = \
            ViewGeometry._activate_and_project(a, p, means, log_scales, quats, opacities, cam_pos, viewmat, full_proj,
                                               fx, fy, cx, cy, img_height, img_width, tile_bounds)
        tail = ShadeTail.forward(t, degrees_to_use, viewdirs, colors_all, depths, normals, bool(one_wave_sh))
        ctx.parts = (a, p, t)
        ctx.pose_meta = (viewmat.shape, viewmat.dtype, full_proj.shape, full_proj.dtype)
        ctx.counts = tuple(len(c.saved_tensors) for c in ctx.parts)
        ctx.save_for_backward(*a.saved_tensors, *p.saved_tensors, *t.saved_tensors)
        for c in ctx.parts:
            c.saved_tensors = ()
        ctx.mark_non_differentiable(radii, num_tiles_hit, packed)
        return xys, depths, radii, conics, num_tiles_hit, opac, tail, normals, packed

    @staticmethod
    def _activate_and_project(a, p, means, log_scales, quats, opacities, cam_pos, viewmat, full_proj, fx, fy, cx, cy,
                              img_height, img_width, tile_bounds):
        """ActivateGaussians.forward + ProjectGaussians.forward (glob_scale 1, default clip) as ONE kernel, gg_view_fwd,
        which also leaves the intersection count and the depth range's partial results behind; `a` / `p` are filled as
        the two forwards fill their ctx (the backwards read them)."""
        dev = _require_hip(means, log_scales, quats, opacities, cam_pos, viewmat, full_proj)
        n = means.shape[0]
        if means.ndim != 2 or means.shape[1] != 3:
            raise ValueError("means3d must have dimensions (N, 3)")
        if tuple(log_scales.shape) != (n, 3) or tuple(quats.shape) != (n, 4) or opacities.numel() != n:
            raise ValueError("expected means (N,3), scales (N,3), quats (N,4), opacities (N,1)")
        if viewmat.numel() < 12 or full_proj.numel() != 16:
            raise ValueError("viewmat must hold >= 12 and projmat exactly 16 elements")
        a.sinks = _sinks_for_all(log_scales, quats, opacities)
        p.sink = _sink_for(means, _dense_f32(means))
        m, s_, q, o = _f32(means), _f32(log_scales), _f32(quats), _f32(opacities)
        c, vm, pm = _f32(cam_pos).reshape(-1), _f32(viewmat), _f32(full_proj)
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
        scales_e, quats_n, opac, viewdirs, normals = f(n, 3), f(n, 4), f(n, 1), f(n, 3), f(n, 3)
        xys, depths, conics = f(n, 2), f(n), f(n, 3)
        axis, radii, num_tiles_hit = i32(n), i32(n), i32(n)
        lib = _lib.load()
        blocks = max((n + 255) // 256, 1)
        parts = i32(3 * blocks)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        packed = _workspace(lib.gg_blend_workspace(n), dev)          # the blend operators' workspace, records packed here
        _lib.check(lib.gg_view_fwd(
            n, _ptr(m), _ptr(s_), _ptr(q), _ptr(o), _ptr(c), _ptr(vm), _ptr(pm), float(fx), float(fy), float(cx),
            float(cy), int(img_height), int(img_width), int(tile_bounds[0]), int(tile_bounds[1]), CLIP_THRESH_DEFAULT,
            _ptr(scales_e), _ptr(quats_n), _ptr(opac), _ptr(viewdirs), _ptr(normals), _ptr(axis), _ptr(xys),
            _ptr(depths), _ptr(radii), _ptr(conics), _ptr(num_tiles_hit), _ptr(total), _ptr(parts), parts.numel() * 4,
            _ptr(packed), packed.numel(), _stream(dev)), "gg_view_fwd")
        a.save_for_backward(q, scales_e, opac, axis)
        a.opacity_shape = tuple(opacities.shape)
        p.scalars = (1.0, float(fx), float(fy), float(cx), float(cy), int(img_height), int(img_width))
        p.save_for_backward(m, scales_e, quats_n, vm, pm, radii, conics)
        _start_count(num_tiles_hit, total, (parts[blocks:2 * blocks], parts[2 * blocks:], blocks) if n > 0 else None)
        return (scales_e, quats_n, opac.reshape(a.opacity_shape), viewdirs, normals, xys, depths, radii, conics,
                num_tiles_hit, packed)

    @staticmethod
    def backward(ctx, v_xys, v_depths, v_radii, v_conics, v_nth, v_opac, v_tail, v_normals, v_packed=None):
        a, p, t = ctx.parts
        saved, k = ctx.saved_tensors, 0
        for c, cnt in zip(ctx.parts, ctx.counts):
            c.saved_tensors = saved[k:k + cnt]
            k += cnt
        q_raw, scales_e, opac, axis = a.saved_tensors
        means, _scales, quats_n, viewmat, projmat, radii, conics = p.saved_tensors
        viewdirs, mask = t.saved_tensors
        dev, n = means.device, means.shape[0]
        sinks_ok = a.sinks is not None and p.sink is not None and t.sink is not None
        fast = sinks_ok and v_depths is None and v_normals is None and v_xys is not None
        if fast:
            base, stride = v_xys.data_ptr(), v_xys.stride(0)
            fast = (stride >= 13 and _is_record_view(v_xys, base, 0, 2, stride, n)
                    and _is_record_view(v_conics, base, 2, 3, stride, n)
                    and _is_record_view(v_opac.reshape(n, 1) if v_opac is not None and v_opac.numel() == n else None,
                                        base, 5, 1, stride, n)
                    and _is_record_view(v_tail, base, 6, 7, stride, n)
                    and (stride % 4 != 0 or base % 16 == 0))
        # the camera's gradient: asked for when viewmat (6) or full_proj (7) requires grad — the camera
        # optimizer's route (plugin.py: viewmat from the adjusted camera_to_worlds, full_proj = projmat @ viewmat)
        pose = ctx.needs_input_grad[6] or ctx.needs_input_grad[7]
        if not fast:
            if pose and not any(ctx.needs_input_grad[:5]):
                # frozen Gaussians (pose.refine_camera): only the depth cotangent of the chain reaches the camera
                vd = torch.zeros(n, device=dev) if v_tail is None else v_tail[:, 3].float()
                vd = vd if v_depths is None else vd + _f32(v_depths)
                return (None,) * 6 + ViewGeometry._pose_only(ctx, p, v_xys, vd, v_conics) + (None,) * 9
            g_t = ShadeTail.backward(t, v_tail if v_tail is not None else torch.zeros(n, 7, device=dev))
            vd = g_t[3] if v_depths is None else g_t[3] + _f32(v_depths)
            vn = g_t[4] if v_normals is None else g_t[4] + _f32(v_normals)
            g_p = ProjectGaussians.backward(p, v_xys, vd, None, v_conics, None, None)
            g_a = ActivateGaussians.backward(a, g_p[1], g_p[3], v_opac, None, vn)
            g_cam = ViewGeometry._pose_only(ctx, p, v_xys, vd, v_conics) if pose else (None, None)
            return (g_p[0], g_a[1], g_a[2], g_a[3], g_t[2], None) + g_cam + (None,) * 9
        lib = _lib.load()
        glob_scale, fx, fy, _cx, _cy, img_height, img_width = p.scalars
        v_rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
        v_ls, v_q, v_o = (k.buffer for k in a.sinks)
        args = (n, C.c_void_p(base), stride, _ptr(mask), _ptr(means), _ptr(scales_e), glob_scale, _ptr(q_raw),
                _ptr(quats_n), _ptr(opac), _ptr(axis), _ptr(viewmat), _ptr(projmat), fx, fy, img_height, img_width,
                _ptr(radii), _ptr(conics), _ptr(v_rgb), _ptr(p.sink.buffer), _ptr(v_ls), _ptr(v_q), _ptr(v_o))
        if pose:
            v_vm, v_pm, ws = _pose_outputs(lib, n, dev)
            _lib.check(lib.gg_view_bwd_pose(*args, _ptr(v_vm), _ptr(v_pm), _ptr(ws), ws.numel(), _stream(dev)),
                       "gg_view_bwd_pose")
            g_cam = ViewGeometry._camera_grads(ctx, v_vm, v_pm)
        else:
            g_cam = (None, None)
            _lib.check(lib.gg_view_bwd(*args, _stream(dev)), "gg_view_bwd")
        # the kernel leaves the SH gradient as its factors: always kept, expanded at once unless more views follow
        t.sink.keep_sh(t.degrees_to_use, t.num_bases, viewdirs, v_rgb)
        for sink in (p.sink, *a.sinks):
            sink.done()
        return (None,) * 6 + g_cam + (None,) * 9

    @staticmethod
    def _pose_only(ctx, p, v_xys, v_depths, v_conics):
        """(v_viewmat, v_full_proj) from the projection's cotangents alone (gg_project_pose_bwd): the fallback branch"""
        means, scales, quats_n, viewmat, projmat, radii, conics = p.saved_tensors
        glob_scale, fx, fy, _cx, _cy, img_height, img_width = p.scalars
        dev, n = means.device, means.shape[0]
        v_xys, xy_stride = _rows_or_zeros(v_xys, n, 2, dev)
        v_conics, conic_stride = _rows_or_zeros(v_conics, n, 3, dev)
        v_depths = _f32(v_depths)
        lib = _lib.load()
        v_vm, v_pm, ws = _pose_outputs(lib, n, dev)
        _lib.check(lib.gg_project_pose_bwd(
            n, _ptr(means), _ptr(scales), glob_scale, _ptr(quats_n), _ptr(viewmat), _ptr(projmat), fx, fy, img_height,
            img_width, _ptr(radii), _ptr(conics), _ptr(v_xys), xy_stride, _ptr(v_depths), _ptr(v_conics), conic_stride,
            _ptr(v_vm), _ptr(v_pm), _ptr(ws), ws.numel(), _stream(dev)), "gg_project_pose_bwd")
        return ViewGeometry._camera_grads(ctx, v_vm, v_pm)

    @staticmethod
    def _camera_grads(ctx, v_vm, v_pm):
        """the 12 + 16 sums in the shapes and dtypes of the viewmat / full_proj the forward was given (a viewmat of more
        than 12 elements: its first 12 were read, the rest gets zeros)"""
        vm_shape, vm_dtype, pm_shape, pm_dtype = ctx.pose_meta
        g_vm = v_vm
        numel = 1
        for d in vm_shape:
            numel *= d
        if numel > 12:
            g_vm = torch.cat((v_vm, torch.zeros(numel - 12, dtype=torch.float32, device=v_vm.device)))
        return (g_vm.reshape(vm_shape).to(vm_dtype) if ctx.needs_input_grad[6] else None,
                v_pm.reshape(pm_shape).to(pm_dtype) if ctx.needs_input_grad[7] else None)


# ------------------------------------------------------------------------------------------------
# several colour arrays from one binning (what the plugin's fused model calls)
# ------------------------------------------------------------------------------------------------
class RasterizeSegments(Function):
    """apply(xys, depths, radii, conics, num_tiles_hit, opacity, img_height, img_width,
             colors_0, background_0, colors_1, background_1, ...) -> (image_0, image_1, ...)

    The blend of K colour arrays (N, C_k) over the SAME Gaussians in one operator: one binning, one
    record packing, one `final_T / final_idx`, ONE set of geometry gradients (v_xy, v_conic, v_opacity
    accumulated by every segment's backward kernel into one record, GG_BWD_ACCUMULATE_GEOM) — what the
    reference's four rasterize calls (:735-784) compute, without their redundancy and without
    concatenating the colours: each array keeps its own storage (a 32-channel feature array keeps its
    128-byte aligned rows and, as a leaf, its gradient sink), each image is its own tensor.
    Images are bit-identical to NDRasterizeGaussians on each array."""

    @staticmethod
    def forward(ctx, xys, depths, radii, conics, num_tiles_hit, opacity, img_height, img_width, splits, *segs):
        if len(segs) < 2 or len(segs) % 2:
            raise ValueError("expected colors_0, background_0[, colors_1, background_1, ...]")
        if xys.ndimension() != 2 or xys.size(1) != 2:
            raise ValueError("xys must have dimensions (N, 2)")
        if opacity.ndimension() != 2 or opacity.size(1) != 1:
            raise ValueError("opacity must have dimensions (N, 1)")
        cols, bgs = list(segs[0::2]), list(segs[1::2])
        dev = _require_hip(xys, depths, radii, conics, num_tiles_hit, opacity, *cols, *bgs)
        n = xys.size(0)
        img_height, img_width = int(img_height), int(img_width)
        for c, b in zip(cols, bgs):
            if c.ndimension() != 2 or c.size(0) != n:
                raise ValueError("colors must have dimensions (N, D)")
            assert b.shape[0] == c.shape[1], f"incorrect shape of background color tensor, expected shape {c.shape[1]}"
        xys_c, conics_c, opacity_c = _f32(xys), _f32(conics), _f32(opacity)
        cols_c, bgs_c = [_f32(c) for c in cols], [_f32(b) for b in bgs]
        ctx.sinks = [_sink_for(c, c.shape[1] > 8 and _dense_f32(c)) for c in cols]
        bins = bin_and_sort_gaussians(xys, depths, radii, num_tiles_hit, img_height, img_width, speculative=True)
        lib = _lib.load()
        # splits may come as (splits, packed): `packed` = a blend workspace that already holds these Gaussians' records
        # (ViewGeometry's last output): the pair forward then skips its packing pass
        packed = None
        if isinstance(splits, tuple) and len(splits) == 2 and (splits[1] is None or isinstance(splits[1], Tensor)) \
                and isinstance(splits[0], tuple):
            splits, packed = splits
        if packed is not None and (packed.dtype != torch.uint8 or packed.numel() < lib.gg_blend_workspace(n)
                                   or packed.device != dev):
            raise ValueError("packed: a uint8 blend workspace of gg_blend_workspace(N) bytes on the operands' device")
        ws = packed if packed is not None else _workspace(lib.gg_blend_workspace(n), dev)
        final_Ts = torch.empty(img_height, img_width, dtype=torch.float32, device=dev)
        final_idx = torch.empty(img_height, img_width, dtype=torch.int32, device=dev)
        outs = [torch.empty(img_height, img_width, c.shape[1], dtype=torch.float32, device=dev) for c in cols_c]
        # a >= 32-channel array carries a <= 8-channel one through its first forward walk
        wide = next((i for i, c in enumerate(cols_c) if c.shape[1] >= 32), None)
        small = next((i for i, c in enumerate(cols_c) if c.shape[1] <= 8), None) if wide is not None else None

        def launch():
            if small is not None and packed is not None:
                _lib.check(lib.gg_blend_fwd_pair_packed(
                    cols_c[wide].shape[1], cols_c[small].shape[1], n, img_height, img_width,
                    _ptr(bins.gaussian_ids_sorted), _ptr(bins.tile_bins), _ptr(cols_c[wide]), _ptr(cols_c[small]),
                    _ptr(bgs_c[wide]), _ptr(bgs_c[small]), _ptr(outs[wide]), _ptr(outs[small]), _ptr(final_Ts),
                    _ptr(final_idx), _ptr(ws), ws.numel(), 0 if (EXACT_FORWARD or _DETERMINISTIC) else 1,
                    _stream(dev)), "gg_blend_fwd_pair_packed")
            elif small is not None:
                pair_fwd = lib.gg_blend_fwd_pair if (EXACT_FORWARD or _DETERMINISTIC) else lib.gg_blend_fwd_pair_fast
                _lib.check(pair_fwd(
                    cols_c[wide].shape[1], cols_c[small].shape[1], n, img_height, img_width,
                    _ptr(bins.gaussian_ids_sorted), _ptr(bins.tile_bins), _ptr(xys_c), _ptr(conics_c),
                    _ptr(cols_c[wide]), _ptr(cols_c[small]), _ptr(opacity_c), _ptr(bgs_c[wide]), _ptr(bgs_c[small]),
                    _ptr(outs[wide]), _ptr(outs[small]), _ptr(final_Ts), _ptr(final_idx), _ptr(ws), ws.numel(),
                    _stream(dev)), "gg_blend_fwd_pair")
            for i, (c, b, o) in enumerate(zip(cols_c, bgs_c, outs)):
                if small is not None and i in (wide, small):
                    continue
                _lib.check(lib.gg_blend_fwd(c.shape[1], n, img_height, img_width, _ptr(bins.gaussian_ids_sorted),
                                            _ptr(bins.tile_bins), _ptr(xys_c), _ptr(conics_c), _ptr(c),
                                            _ptr(opacity_c), _ptr(b), _ptr(o), _ptr(final_Ts), _ptr(final_idx),
                                            _ptr(ws), ws.numel(), _stream(dev)), "gg_blend_fwd")

        visible = _blend_with_lists(bins, launch)
        ctx.num_intersects = bins.num_intersects
        ctx.img = (img_height, img_width)
        ctx.opacity_shape = tuple(opacity.shape)
        ctx.nseg = len(cols_c)
        # splits: {segment index: channel counts} — that segment's image is returned as several images (views of
        # one buffer) and its cotangents come back separately (and are handed to the kernel as they are)
        splits = dict(splits or {})
        out_map = []
        for i, c in enumerate(cols_c):
            sizes = list(splits.get(i, [c.shape[1]]))
            if sum(sizes) != c.shape[1] or min(sizes) < 1:
                raise ValueError("split sizes must be positive and add up to the segment's channels")
            start = 0
            for sz in sizes:
                out_map.append((i, start, start + sz))
                start += sz
        ctx.out_map = out_map
        if not visible:
            outs = [torch.ones(img_height, img_width, c.shape[1], device=dev) * b for c, b in zip(cols_c, bgs_c)]
            ctx.save_for_backward(xys_c, conics_c, opacity_c, *cols_c)
        else:
            ctx.save_for_backward(xys_c, conics_c, opacity_c, bins.gaussian_ids_sorted, bins.tile_bins, final_Ts,
                                  final_idx, ws, *cols_c, *bgs_c)
        return tuple(outs[i] if (e - b) == outs[i].shape[2] else outs[i][..., b:e] for i, b, e in out_map)

    @staticmethod
    def backward(ctx, *v_parts):
        k = ctx.nseg
        img_height, img_width = ctx.img
        if ctx.num_intersects < 1:
            xys, conics, opacity = ctx.saved_tensors[:3]
            cols = ctx.saved_tensors[3:]
            grads = []
            for c in cols:
                grads += [torch.zeros_like(c), None]
            return (torch.zeros_like(xys), None, None, torch.zeros_like(conics), None,
                    torch.zeros_like(opacity).reshape(ctx.opacity_shape), None, None, None, *grads)
        xys, conics, opacity, ids_sorted, tile_bins, final_Ts, final_idx, ws = ctx.saved_tensors[:8]
        cols, bgs = ctx.saved_tensors[8:8 + k], ctx.saved_tensors[8 + k:8 + 2 * k]
        dev, n = xys.device, xys.shape[0]
        lib = _lib.load()
        # one record per Gaussian for the geometry gradients of ALL segments; the colours of the
        # narrowest small segment (<= 8 channels) ride in the same record (one cache line per Gaussian)
        small = [i for i in range(k) if cols[i].shape[1] <= 8]
        rider = min(small, key=lambda i: cols[i].shape[1]) if small else None
        gwidth = 6 + (cols[rider].shape[1] if rider is not None else 0)
        wide = next((i for i in range(k) if cols[i].shape[1] >= 32), None)
        # The pair walk: 16-float records on a 64-byte boundary — geometry sums and the rider's colour gradients of a
        # Gaussian then leave the kernel as ONE atomic request (csrc/blend2.hip, MG); other walks: dense records
        gstride = 16 if (rider is not None and wide is not None and not _DETERMINISTIC and gwidth <= 16) else gwidth
        rec_g = torch.empty(n, gstride, dtype=torch.float32, device=dev)
        v_xy, v_conic, v_opacity = rec_g[:, 0:2], rec_g[:, 2:5], rec_g[:, 5:6]
        order = ([rider] if rider is not None else []) + [i for i in range(k) if i != rider]
        grads = [None] * k
        first = True

        def parts(i):
            """cotangents of segment i as [(image, channels)] in channel order"""
            out = []
            for (seg, b, e), v in zip(ctx.out_map, v_parts):
                if seg != i:
                    continue
                if v is None:
                    v = torch.zeros(img_height, img_width, e - b, dtype=torch.float32, device=dev)
                out.append((_f32(v), e - b))
            return out

        def cotangent(i):
            p = parts(i)
            return p[0][0] if len(p) == 1 else torch.cat([v for v, _ in p], dim=-1)

        # a >= 32-channel array carries the rider through its first backward walk (gg_blend_bwd_pair): one
        # walk computes alpha, T and the geometry gradients of both arrays
        if rider is not None and wide is not None and not _DETERMINISTIC:
            sink = ctx.sinks[wide]
            flags = 1
            if sink is not None:
                v_colors = sink.buffer
                flags |= 2
            else:
                v_colors = torch.empty(n, cols[wide].shape[1], dtype=torch.float32, device=dev)
            vo_w, rp = cotangent(wide), parts(rider)
            if len(rp) > 3:
                rp = [(cotangent(rider), cols[rider].shape[1])]
            part_ptrs = (C.c_void_p * len(rp))(*[_ptr(v) for v, _ in rp])
            part_chs = (C.c_int * len(rp))(*[c for _, c in rp])
            _lib.check(lib.gg_blend_bwd_pair(
                cols[wide].shape[1], cols[rider].shape[1], n, img_height, img_width, _ptr(ids_sorted),
                _ptr(tile_bins), _ptr(xys), _ptr(conics), _ptr(cols[wide]), _ptr(cols[rider]), _ptr(opacity),
                _ptr(bgs[wide]), _ptr(bgs[rider]), _ptr(final_Ts), _ptr(final_idx), _ptr(vo_w), part_ptrs,
                part_chs, len(rp), _ptr(v_xy), _ptr(v_conic), _ptr(v_colors), _ptr(rec_g[:, 6:gwidth]),
                _ptr(v_opacity), gstride, 0, gstride, _ptr(ws), ws.numel(), flags, _stream(dev)),
                "gg_blend_bwd_pair")
            grads[rider] = rec_g[:, 6:gwidth]
            if flags & 2:
                sink.done()
            else:
                grads[wide] = v_colors
            order = [i for i in range(k) if i not in (wide, rider)]
            first = False
        for i in order:
            ch = cols[i].shape[1]
            v_out = cotangent(i)
            flags = 1 | (0 if first else 4)
            sink = ctx.sinks[i]
            if i == rider:
                v_colors, cstride = rec_g[:, 6:gwidth], gstride
            elif sink is not None:
                v_colors, cstride = sink.buffer, 0
                flags |= 2
            else:
                v_colors, cstride = torch.empty(n, ch, dtype=torch.float32, device=dev), 0
            _blend_bwd(lib, ch, n, img_height, img_width, ids_sorted, tile_bins, xys, conics, cols[i], opacity,
                       bgs[i], final_Ts, final_idx, v_out, v_xy, v_conic, v_colors, v_opacity, gstride, cstride,
                       ws, flags, ctx.num_intersects)
            first = False
            if flags & 2:
                sink.done()
            else:
                grads[i] = v_colors
        seg_grads = []
        for g in grads:
            seg_grads += [g, None]
        return (v_xy, None, None, v_conic, None, v_opacity.reshape(ctx.opacity_shape), None, None, None, *seg_grads)


def rasterize_segments(xys, depths, radii, conics, num_tiles_hit, opacity, img_height, img_width, segments,
                       packed: Optional[Tensor] = None):
    """segments: sequence of (colors (N, C_k), background (C_k,)[, split sizes]) -> list of images (H, W, C_k);
    a segment given with split sizes (e.g. [3, 1, 3] for rgb | depth | normal) comes back as that many images
    (views of one buffer, channel-sliced), and their cotangents go to the backward kernel without a concatenation."""
    flat, splits = [], {}
    for i, seg in enumerate(segments):
        flat += [seg[0], seg[1]]
        if len(seg) > 2 and seg[2] is not None:
            splits[i] = tuple(int(x) for x in seg[2])
    spec = tuple(sorted(splits.items()))
    return list(RasterizeSegments.apply(xys, depths, radii, conics, num_tiles_hit, opacity, img_height,
                                        img_width, (spec, packed) if packed is not None else spec, *flat))


# ------------------------------------------------------------------------------------------------
# quat_to_rotmat (gsplat._torch_impl; reference gaussian_splatting.py:516,614, scripts/update.py:204,229)
# ------------------------------------------------------------------------------------------------
class _QuatToRotmat(Function):
    @staticmethod
    def forward(ctx, quat: Tensor) -> Tensor:
        dev = _require_hip(quat)
        q = _f32(quat).reshape(-1, 4)
        rot = torch.empty(q.shape[0], 9, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().gg_quat_to_rotmat_fwd(q.shape[0], _ptr(q), _ptr(rot), _stream(dev)),
                   "gg_quat_to_rotmat_fwd")
        ctx.save_for_backward(q)
        ctx.in_shape, ctx.in_dtype = quat.shape, quat.dtype
        return rot.reshape(quat.shape[:-1] + (3, 3))

    @staticmethod
    def backward(ctx, v_rot: Tensor):
        (q,) = ctx.saved_tensors
        dev = q.device
        g = _f32(v_rot).reshape(-1, 9)
        v_q = torch.empty_like(q)
        _lib.check(_lib.load().gg_quat_to_rotmat_bwd(q.shape[0], _ptr(q), _ptr(g), _ptr(v_q),
                                                     _stream(dev)), "gg_quat_to_rotmat_bwd")
        return v_q.reshape(ctx.in_shape).to(ctx.in_dtype)


def quat_to_rotmat(quat: Tensor) -> Tensor:
    """Rotation matrices (...,3,3) of wxyz quaternions (normalised first), differentiable.
    gsplat's is ~35 torch elementwise launches forward and ~70 backward on strided views; here
    one HIP kernel each way (gg_quat_to_rotmat_fwd/bwd)."""
    if quat.shape[-1] != 4:
        raise ValueError(f"quat must have dimensions (..., 4), got {tuple(quat.shape)}")
    return _QuatToRotmat.apply(quat)


# ------------------------------------------------------------------------------------------------
# RigidMove: a subset of the Gaussians moved by a pose that is itself a tensor
# ------------------------------------------------------------------------------------------------
def _quat_mul(a: Tensor, b: Tensor) -> Tensor:
    """Hamilton product of wxyz quaternions, every component in the order of include/gg_raster.h"""
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack((w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2), -1)


def rigid_move_torch(means: Tensor, quats: Tensor, mask: Optional[Tensor], rt: Tensor, qt: Tensor):
    """gg_rigid_fwd's formulas as a torch composite on any device: fp64 inside, each output rounded once to the
    input's dtype, rows not selected passed through.  What RigidMove runs on CPU tensors (the host tests and the
    oracle-backed routes) and what tools/rigid_bench.py times the kernels against."""
    rt64 = rt.reshape(3, 4).double()
    m, q = means.double(), quats.double()
    R, t = rt64[:, :3], rt64[:, 3]
    moved = ((R[:, 0] * m[:, 0:1] + R[:, 1] * m[:, 1:2]) + R[:, 2] * m[:, 2:3]) + t
    turned = _quat_mul(qt.reshape(1, 4).double(), q)
    moved, turned = moved.to(means.dtype), turned.to(quats.dtype)
    if mask is None:
        return moved, turned
    sel = (mask != 0)[:, None]
    return torch.where(sel, moved, means), torch.where(sel, turned, quats)


class RigidMoveFunction(Function):
    """(means, quats, mask, rt, qt) -> (means', quats') on gg_rigid_fwd / gg_rigid_bwd.  The pose's gradient is the
    kernels' ordered fp64 sum: the same inputs give the same bits."""

    @staticmethod
    def forward(ctx, means: Tensor, quats: Tensor, mask: Optional[Tensor], rt: Tensor, qt: Tensor):
        dev = _require_hip(means, quats, rt, qt, *([mask] if mask is not None else []))
        m, q = _f32(means), _f32(quats)
        n = m.shape[0]
        if m.ndim != 2 or m.shape[1] != 3 or q.shape != (n, 4):
            raise ValueError(f"means must be (N, 3) and quats (N, 4), got {tuple(m.shape)} and {tuple(q.shape)}")
        if rt.numel() != 12 or qt.numel() != 4:
            raise ValueError(f"rt must hold 12 numbers and qt 4, got {tuple(rt.shape)} and {tuple(qt.shape)}")
        if mask is not None:
            if mask.shape != (n,) or mask.dtype not in (torch.uint8, torch.bool):
                raise ValueError(f"mask must be a uint8 or bool (N,) tensor, got {mask.dtype} {tuple(mask.shape)}")
            mask = mask.contiguous().view(torch.uint8)
        rt_c, qt_c = _f32(rt.detach()).reshape(12), _f32(qt.detach()).reshape(4)
        m_out, q_out = torch.empty_like(m), torch.empty_like(q)
        _lib.check(_lib.load().gg_rigid_fwd(n, _ptr(m), _ptr(q), _ptr(mask), _ptr(rt_c), _ptr(qt_c), _ptr(m_out),
                                            _ptr(q_out), _stream(dev)), "gg_rigid_fwd")
        ctx.save_for_backward(m, q, mask, rt_c, qt_c)
        ctx.shapes = (rt.shape, qt.shape, rt.dtype, qt.dtype, means.dtype, quats.dtype)
        return m_out.to(means.dtype), q_out.to(quats.dtype)

    @staticmethod
    def backward(ctx, g_means, g_quats):
        m, q, mask, rt_c, qt_c = ctx.saved_tensors
        rt_shape, qt_shape, rt_dtype, qt_dtype, m_dtype, q_dtype = ctx.shapes
        dev, n = m.device, m.shape[0]
        lib = _lib.load()
        rows = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]     # frozen Gaussians: the pose-only pass
        g_m = None if g_means is None else _f32(g_means)
        g_q = None if g_quats is None else _f32(g_quats)
        v_m = torch.empty_like(m) if rows else None
        v_q = torch.empty_like(q) if rows else None
        v_pose = torch.empty(16, dtype=torch.float32, device=dev)
        ws = _workspace(lib.gg_rigid_bwd_workspace(n), dev)
        _lib.check(lib.gg_rigid_bwd(n, _ptr(m), _ptr(q), _ptr(mask), _ptr(rt_c), _ptr(qt_c), _ptr(g_m), _ptr(g_q),
                                    _ptr(v_m), _ptr(v_q), _ptr(v_pose), C.c_void_p(v_pose.data_ptr() + 48), _ptr(ws),
                                    ws.numel(), _stream(dev)), "gg_rigid_bwd")
        return (v_m.to(m_dtype) if ctx.needs_input_grad[0] else None,
                v_q.to(q_dtype) if ctx.needs_input_grad[1] else None, None,
                v_pose[:12].reshape(rt_shape).to(rt_dtype) if ctx.needs_input_grad[3] else None,
                v_pose[12:].reshape(qt_shape).to(qt_dtype) if ctx.needs_input_grad[4] else None)


def RigidMove(means: Tensor, quats: Tensor, mask: Optional[Tensor], rt: Tensor, qt: Tensor) -> Tuple[Tensor, Tensor]:
    """Move the rows of `means` (N, 3) and `quats` (N, 4, wxyz) that `mask` (N,) uint8 / bool selects (None: every
    row) by the pose rt = [R | t] (12 numbers, row-major) and qt, the quaternion of R: means' = R x + t,
    quats' = qt (x) q, not normalised; the other rows pass through.  Differentiable in means, quats, rt and qt.
    On a HIP device one kernel each way (RigidMoveFunction); CPU tensors run the torch composite of the same formulas
    (rigid_move_torch) — that route is for the host tests and the oracle-backed operators, not a fallback: a HIP
    tensor never takes it."""
    if means.device.type == "cpu":
        return rigid_move_torch(means, quats, mask, rt, qt)
    return RigidMoveFunction.apply(means, quats, mask, rt, qt)
