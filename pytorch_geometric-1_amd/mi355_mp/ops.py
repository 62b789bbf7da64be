"""Torch-facing ops over the native engine (autograd included).

Every function here launches HIP kernels from libmi355_mp.so on the current
stream; inputs must already live on the GPU.  Backward passes reuse the same
kernels on the transposed CSR.

Reference semantics (all [U], restated from torch_scatter 2.0.4 /
torch_geometric 1.4.3; see oracle/ for the CPU restatement used as checker):
  * sum/add   : scatter_sum = zeros(...).scatter_add_(0, index, src)
  * mean      : scatter_sum / count.clamp(1)
  * max/min   : (out, arg); strict compare, first edge wins ties, empty row
                -> (0, src.size(0)); scatter_(...) also masks <-10000 / >10000
"""
import os

import torch

from . import _lib
from .graph import _Cache, csr_for_index, in_csr_order

_REDUCES = ("sum", "add", "mean", "max", "min")


def _any_2d(x, what):
    """A 2-D row-major tensor of a dtype the native reductions take (fp32 hot
    path; float64 / float16 / bfloat16 / int64 breadth path, mp_segment_reduce)."""
    if x.dtype not in _lib.MP_DTYPE:
        raise TypeError("mi355_mp: %s dtype %s is not supported (float32, float64, float16, bfloat16, int64)"
                        % (what, x.dtype))
    if x.dim() != 2:
        raise ValueError("mi355_mp: %s must be 2-D [rows, features]" % what)
    if x.stride(1) != 1 or x.stride(0) < max(x.shape[1], 1):
        x = x.contiguous()
    return x


def _aggregate_any(csr, gather, src, reduce, flags, out=None):
    """mp_segment_reduce: any supported dtype, every row in edge order (not
    split).  Returns (out, arg_or_None)."""
    nat = _lib.native()
    F = src.shape[1]
    dev = src.device
    if out is None:
        out = torch.empty((csr.n_rows, F), dtype=src.dtype, device=dev)
    arg = torch.empty((csr.n_rows, F), dtype=torch.int64, device=dev) if reduce in ("max", "min") else None
    if csr.n_rows == 0 or F == 0:
        return out, arg
    nat.mp_segment_reduce(csr.struct(gather), _lib.MP_DTYPE[src.dtype], src.data_ptr(), src.stride(0), F,
                          _lib.MP_REDUCE[reduce], flags, out.data_ptr(), out.stride(0), _lib.ptr(arg),
                          _lib.stream_ptr(dev))
    return out, arg


def _f32_2d(x, what):
    if x.dtype != torch.float32:
        raise TypeError("mi355_mp: %s must be float32 (got %s)" % (what, x.dtype))
    if x.dim() != 2:
        raise ValueError("mi355_mp: %s must be 2-D [rows, features]" % what)
    if x.stride(1) != 1:
        x = x.contiguous()
    return x


# Unweighted max / min over x[col] read each (row, column) pair once: from the
# (FIRST_OCCURRENCE_AFTER + 1)-th such aggregation over one CSR on, the CSR's
# first-occurrence form (graph.CSR.first_occurrences: bit-identical results,
# no repeated gathers) is built once and used.  A one-off aggregation never
# pays for its sort; a layer reused every epoch does.  None disables it.
FIRST_OCCURRENCE_AFTER = 2


def _max_csr(csr):
    if FIRST_OCCURRENCE_AFTER is None:
        return csr
    n = getattr(csr, "_max_uses", 0) + 1
    csr._max_uses = n
    return csr.first_occurrences() if n > FIRST_OCCURRENCE_AFTER else csr


def _aggregate(csr, gather, x, w_csr, reduce, flags, bias, out=None, stages=_lib.MP_STAGE_ALL, slab=None,
               arg=None):
    """Launch mp_aggregate_f32; returns (out, arg_or_None)."""
    nat = _lib.native()
    if reduce in ("max", "min") and w_csr is None and gather == "other" and stages == _lib.MP_STAGE_ALL:
        csr = _max_csr(csr)
    F = x.shape[1]
    dev = x.device
    if out is None:
        out = torch.empty((csr.n_rows, F), dtype=torch.float32, device=dev)
    is_arg = reduce in ("max", "min")
    if is_arg and arg is None:
        arg = torch.empty((csr.n_rows, F), dtype=torch.int64, device=dev)
    if csr.n_rows == 0 or F == 0:
        return out, arg
    g = csr.struct(gather)
    red = _lib.MP_REDUCE[reduce]
    sb = nat.mp_aggregate_slab_bytes(g, F, red)
    if slab is None or slab.numel() < sb:
        slab = torch.empty(sb, dtype=torch.uint8, device=dev)
    nat.mp_aggregate_f32(g, _lib.ptr(w_csr), x.data_ptr(), x.stride(0), F, red, flags, _lib.ptr(bias), out.data_ptr(),
                         out.stride(0), _lib.ptr(arg), slab.data_ptr(), sb, stages, _lib.stream_ptr(dev))
    return out, arg


def aggregate_tiles(csr, gather, x, w_csr, F, out, reduce="sum", flags=0, bias=None, x_tiles=None, out_tiles=None,
                    slab=None, stages=_lib.MP_STAGE_ALL, bias_rows=None):
    """One sum / mean launch (mp_aggregate_tiles_f32) over operands held
    tile-major: x_tiles / out_tiles = (width, stride in elements) when x / out
    is a [T, rows, width] buffer (feature f of row r at
    [f // width][r][f % width]), None when row-major (then x / out is a 2-D
    tensor and its row stride is used).  bias_rows: None, or int32 [rows]
    flags -- the bias goes only to rows whose flag is nonzero.  Bitwise the
    arithmetic of _aggregate on the same values laid out row-major.  Returns
    out."""
    nat = _lib.native()
    dev = out.device
    if csr.n_rows == 0:
        return out
    g = csr.struct(gather)
    red = _lib.MP_REDUCE[reduce]
    sb = nat.mp_aggregate_slab_bytes(g, F, red)
    if slab is None or slab.numel() < sb:
        slab = torch.empty(sb, dtype=torch.uint8, device=dev)
    xw, xs = x_tiles if x_tiles is not None else (0, 0)
    ow, os_ = out_tiles if out_tiles is not None else (0, 0)
    ldx = 0 if x_tiles is not None else x.stride(0)
    ldo = 0 if out_tiles is not None else out.stride(0)
    nat.mp_aggregate_tiles_f32(g, _lib.ptr(w_csr), x.data_ptr() if x.numel() else None, ldx, xw, xs, F, red, flags,
                               _lib.ptr(bias), _lib.ptr(bias_rows), out.data_ptr(), ldo, ow, os_, slab.data_ptr(), sb,
                               stages, _lib.stream_ptr(dev))
    return out


def gather_rows(x, idx):
    """out = x[idx] via the native row gather (no autograd; see GatherRows)."""
    nat = _lib.native()
    x = _any_2d(x, "x")
    idx = idx.to(torch.int64).contiguous()
    out = torch.empty((idx.numel(), x.shape[1]), dtype=x.dtype, device=x.device)
    if idx.numel() and x.shape[1]:
        if x.dtype == torch.float32:
            nat.mp_gather_rows_f32(x.data_ptr(), x.stride(0), idx.data_ptr(), idx.numel(), x.shape[1], out.data_ptr(),
                                   out.stride(0), _lib.stream_ptr(x.device))
        else:
            nat.mp_gather_rows_any(x.element_size(), x.data_ptr(), x.stride(0), idx.data_ptr(), idx.numel(), x.shape[1],
                                   out.data_ptr(), out.stride(0), _lib.stream_ptr(x.device))
    return out


def col_sums(g):
    """sum over rows of a [n, F] fp32 gradient (a bias gradient): native
    per-block partials (mp_col_sums_f32) where the row fits 256 features,
    else torch's reduction."""
    n, F = g.shape
    if g.is_cuda and 0 < F <= 256 and F % 4 == 0 and g.stride(1) == 1 and g.stride(0) % 4 == 0 \
            and g.data_ptr() % 16 == 0 and g.dtype == torch.float32:
        nat = _lib.native()
        part = torch.empty((int(nat.mp_gat_bwd_blocks(n)), F), dtype=torch.float32, device=g.device)
        nat.mp_col_sums_f32(g.data_ptr(), g.stride(0), n, F, part.data_ptr(), _lib.nbytes(part),
                            _lib.stream_ptr(g.device))
        return part.sum(0)
    return g.sum(0)


def arg_backward(graph, arg, g, n_src, edge_weight=None, x=None, want_gx=True, want_gw=False):
    """ScatterMax / ScatterMin backward of the fused message w_e * x[src_e]
    (torch_scatter 2.0.4 [U8]: grad_msg = zeros(E+1, F).scatter_(0, arg, g)[:E],
    then the message's backward and index_select's backward, an index_add_ by
    source in edge order), deterministic and in the reference's order: a winner
    bit mask in the transposed CSR's slot order, then one pass over the
    transposed CSR that adds each source row's winning terms slot by slot
    (mp_scatter_arg_backward_csr_f32) -- no float atomics.  `arg` holds original
    edge ids of graph.dst's edges (E = no edge).  Returns (gx or None, gw or None)."""
    nat = _lib.native()
    dev = g.device
    st = _lib.stream_ptr(dev)
    src = graph.src
    E = src.n_edges
    F = g.shape[1]
    inv = src.inverse_eid()
    W = int(nat.mp_arg_mask_words(F))
    mask = torch.empty(max(E * W, 2), dtype=torch.int32, device=dev)
    nat.mp_arg_winner_mask(arg.data_ptr(), g.shape[0], F, E, inv.data_ptr(), mask.data_ptr(), _lib.nbytes(mask), st)
    w = edge_weight.to(torch.float32).contiguous() if edge_weight is not None else None
    gx = gw = None
    if want_gx:
        gx = torch.empty((int(n_src), F), dtype=torch.float32, device=dev)
        nat.mp_scatter_arg_backward_csr_f32(src.struct("other"), mask.data_ptr(), _lib.nbytes(mask), g.data_ptr(),
                                            g.stride(0), F, _lib.ptr(w), gx.data_ptr(), gx.stride(0), st)
    if want_gw:
        ei = graph._edge_index()
        srcs = ei[graph.j].contiguous()
        dsts = ei[graph.i].contiguous()
        gw = torch.empty(max(E, 1), dtype=torch.float32, device=dev)[:E]
        nat.mp_scatter_arg_grad_w_f32(srcs.data_ptr(), dsts.data_ptr(), E, inv.data_ptr(), mask.data_ptr(),
                                      _lib.nbytes(mask), F, g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0),
                                      gw.data_ptr(), st)
    return gx, gw


# ---------------------------------------------------------------------------
# fused gather -> weight -> reduce over a Graph (MessagePassing fast path)
# ---------------------------------------------------------------------------

class _FusedPropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, edge_weight, bias, graph, edge_index, reduce, pyg_mask, weight_csr):
        csr = graph.dst
        w_csr = weight_csr
        if w_csr is None and edge_weight is not None:
            w_csr = in_csr_order(csr, edge_weight)
        is_arg = reduce in ("max", "min")
        need_mask_grad = is_arg and pyg_mask and ctx.needs_input_grad[0]
        flags = _lib.MP_FLAG_PYG_MASK if (pyg_mask and not need_mask_grad) else 0
        fuse_bias = bias if not need_mask_grad else None
        out, arg = _aggregate(csr, "other", x, w_csr, reduce, flags, fuse_bias)
        keep = None
        if need_mask_grad:
            keep = ~((out < -10000) if reduce == "max" else (out > 10000))
            out = out.masked_fill(~keep, 0.0)
            if bias is not None:
                out = out + bias
        ctx.graph = graph
        ctx.reduce = reduce
        ctx.n_src = x.shape[0]
        ctx.save_for_backward(x, edge_weight, edge_index, arg, keep)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, edge_weight, edge_index, arg, keep = ctx.saved_tensors
        graph, reduce = ctx.graph, ctx.reduce
        grad_out = grad_out.contiguous()
        gx = gw = gb = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = col_sums(grad_out)
        if reduce in ("max", "min"):
            want_w = ctx.needs_input_grad[1] and edge_weight is not None
            if ctx.needs_input_grad[0] or want_w:
                # message = w_e * x[src_e] at the argmax edge e: d x[src_e] += w_e g,
                # d w_e += <g, x[src_e]> over the features whose argmax is e
                g = (grad_out * keep if keep is not None else grad_out).contiguous()
                gx, gw = arg_backward(graph, arg, g, ctx.n_src, edge_weight, x, ctx.needs_input_grad[0], want_w)
                if gw is not None and gw.dtype != edge_weight.dtype:
                    gw = gw.to(edge_weight.dtype)
            return gx, gw, gb, None, None, None, None, None
        g = grad_out
        if reduce == "mean":
            deg = graph.dst.degree().clamp(min=1).to(torch.float32)
            g = g / deg.view(-1, 1)
        if ctx.needs_input_grad[0]:
            src = graph.src  # transposed CSR: rows = source nodes, gathers destination rows
            w_src = in_csr_order(src, edge_weight) if edge_weight is not None else None
            gx, _ = _aggregate(src, "other", g, w_src, "sum", 0, None)
        if ctx.needs_input_grad[1] and edge_weight is not None:
            gw = _edge_dot(graph.dst, g.contiguous(), x).to(edge_weight.dtype)
        return gx, gw, gb, None, None, None, None, None


def _edge_dot(csr, g, x):
    """d w_e = <g[dst_e], x[src_e]> for every edge, in original edge order: one
    CSR SDDMM over the destination CSR (mp_gat_sddmm_f32 with one head of width
    F), then a permutation by eid -- no [E, F] gathers of x_j and g_i."""
    E = csr.n_edges
    F = g.shape[1]
    dev = g.device
    out = torch.zeros(E, dtype=torch.float32, device=dev)
    if E == 0 or F == 0:
        return out
    sr = csr.slot_rows()
    d = torch.empty(E, dtype=torch.float32, device=dev)
    _lib.native().mp_gat_sddmm_f32(csr.struct("other"), sr.data_ptr(), g.data_ptr(), g.stride(0), x.data_ptr(),
                                   x.stride(0), 1, F, d.data_ptr(), _lib.stream_ptr(dev))
    out[csr.eid[:E].long()] = d
    return out


def fused_propagate(graph, x, edge_index, edge_weight=None, reduce="sum", bias=None, pyg_mask=False,
                    weight_csr=None):
    """out[i] = REDUCE_{e : index[e] == i} (w[e] * x[other[e]]) (+ bias).

    The fused form of ``propagate`` for message(x_j) / message(x_j, norm)
    (PyG 1.4.3 MessagePassing [U1] + GCNConv.message [U5]).
    """
    if reduce not in _REDUCES:
        raise ValueError("unknown reduce %r" % (reduce,))
    reduce = "sum" if reduce == "add" else reduce
    _lib.require_device(x, edge_index, edge_weight, bias)
    x = _f32_2d(x, "x")
    return _FusedPropagate.apply(x, edge_weight, bias, graph, edge_index, reduce, pyg_mask, weight_csr)


# ---------------------------------------------------------------------------
# materialised-message path (torch_scatter semantics)
# ---------------------------------------------------------------------------

class _SegmentReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, index, dim_size, reduce, pyg_mask):
        csr = csr_for_index(index, dim_size)
        need_mask_grad = pyg_mask and reduce in ("max", "min") and ctx.needs_input_grad[0]
        flags = _lib.MP_FLAG_PYG_MASK if (pyg_mask and not need_mask_grad) else 0
        if src.dtype == torch.float32:
            out, arg = _aggregate(csr, "eid", src, None, reduce, flags, None)
        else:
            out, arg = _aggregate_any(csr, "eid", src, reduce, flags)
        ctx.reduce = reduce
        ctx.csr = csr
        ctx.n_src = src.shape[0]
        keep = None
        if need_mask_grad:
            keep = ~((out < -10000) if reduce == "max" else (out > 10000))
            out = out.masked_fill(~keep, 0.0)
        ctx.save_for_backward(index, arg, keep)
        if arg is not None:
            ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, grad_out, _grad_arg=None):
        index, arg, keep = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        reduce = ctx.reduce
        if reduce in ("max", "min"):
            nat = _lib.native()
            g = (grad_out * keep if keep is not None else grad_out).contiguous()
            gs = torch.zeros((ctx.n_src, g.shape[1]), dtype=g.dtype, device=g.device)
            if g.dtype == torch.float32:
                nat.mp_scatter_arg_backward_f32(g.data_ptr(), arg.data_ptr(), g.shape[0], g.shape[1], ctx.n_src,
                                                gs.data_ptr(), gs.stride(0), _lib.stream_ptr(g.device))
            else:
                nat.mp_scatter_arg_any(g.element_size(), g.data_ptr(), arg.data_ptr(), g.shape[0], g.shape[1],
                                       ctx.n_src, gs.data_ptr(), gs.stride(0), _lib.stream_ptr(g.device))
            return gs, None, None, None, None
        g = grad_out
        if reduce == "mean":
            g = g / ctx.csr.degree().clamp(min=1).to(g.dtype).view(-1, 1)
        return gather_rows(g, index), None, None, None, None


def segment_reduce(src, index, dim_size, reduce="sum", pyg_mask=False):
    """torch_scatter.scatter_{sum,mean,max,min}(src, index, 0, dim_size=...) on 2-D src.

    Returns (out, arg) with arg None for sum/mean.
    """
    if reduce not in _REDUCES:
        raise ValueError("unknown reduce %r" % (reduce,))
    reduce = "sum" if reduce == "add" else reduce
    _lib.require_device(src, index)
    src = _any_2d(src, "src")
    if index.dim() != 1 or index.numel() != src.shape[0]:
        raise ValueError("mi355_mp: index must be 1-D with src.size(0) entries")
    return _SegmentReduce.apply(src, index, int(dim_size), reduce, pyg_mask)


def _reduce_into_native(src, index, out, reduce):
    csr = csr_for_index(index, out.shape[0])
    if src.dtype == torch.float32:
        res, arg = _aggregate(csr, "eid", src, None, reduce, _lib.MP_FLAG_INIT_FROM_OUT, None, out=out)
    else:
        res, arg = _aggregate_any(csr, "eid", src, reduce, _lib.MP_FLAG_INIT_FROM_OUT, out=out)
    return res, arg, csr


class _SegmentReduceInto(torch.autograd.Function):
    """torch_scatter 2.0.4's ``out=`` forms with autograd, as upstream
    differentiates them: scatter_sum is ``out.scatter_add_(dim, index, src)``
    (d src = gather(g), d out = g), scatter_mean divides that by the clamped
    count in place (d src = gather(g / count), d out = g / count), and the
    C++ ScatterMax / ScatterMin give src its winners' gradients and out none.
    Out of place here (the result a fresh tensor); segment_reduce_into copies
    it into the caller's out."""

    @staticmethod
    def forward(ctx, src, index, out_old, reduce):
        res = out_old.clone(memory_format=torch.contiguous_format)
        res, arg, csr = _reduce_into_native(src, index, res, reduce)
        ctx.reduce, ctx.csr, ctx.n_src = reduce, csr, src.shape[0]
        ctx.save_for_backward(index, arg)
        if arg is not None:
            ctx.mark_non_differentiable(arg)
        return res, arg

    @staticmethod
    def backward(ctx, g, _grad_arg=None):
        index, arg = ctx.saved_tensors
        g = g.contiguous()
        if ctx.reduce in ("max", "min"):
            nat = _lib.native()
            gs = torch.zeros((ctx.n_src, g.shape[1]), dtype=g.dtype, device=g.device)
            if g.dtype == torch.float32:
                nat.mp_scatter_arg_backward_f32(g.data_ptr(), arg.data_ptr(), g.shape[0], g.shape[1], ctx.n_src,
                                                gs.data_ptr(), gs.stride(0), _lib.stream_ptr(g.device))
            else:
                nat.mp_scatter_arg_any(g.element_size(), g.data_ptr(), arg.data_ptr(), g.shape[0], g.shape[1],
                                       ctx.n_src, gs.data_ptr(), gs.stride(0), _lib.stream_ptr(g.device))
            return gs, None, None, None
        if ctx.reduce == "mean":
            g = g / ctx.csr.degree().clamp(min=1).to(g.dtype).view(-1, 1)
        return gather_rows(g, index), None, g, None


def segment_reduce_into(src, index, out, reduce="sum"):
    """torch_scatter ``out=`` semantics: reduce into (and return) the given out
    tensor; differentiable in src and out as upstream (_SegmentReduceInto)."""
    reduce = "sum" if reduce == "add" else reduce
    _lib.require_device(src, index, out)
    src = _any_2d(src, "src")
    # (a one-feature out may carry any stride on its size-1 dim: torch calls it contiguous)
    if out.dtype != src.dtype or out.dim() != 2 or (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError("mi355_mp: out must be a row-major [dim_size, F] tensor of src's dtype")
    if torch.is_grad_enabled() and (src.requires_grad or out.requires_grad):
        res, arg = _SegmentReduceInto.apply(src, index, out, reduce)
        out.copy_(res)
        return out, arg
    res, arg, _ = _reduce_into_native(src, index, out, reduce)
    return res, arg


class GatherRows(torch.autograd.Function):
    """x[idx] with backward = segment-sum of the row gradients by idx (native)."""

    @staticmethod
    def forward(ctx, x, idx):
        ctx.n = x.shape[0]
        ctx.save_for_backward(idx)
        return gather_rows(x, idx)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        csr = csr_for_index(idx, ctx.n)
        g = g.contiguous()
        if g.dtype == torch.float32:
            gx, _ = _aggregate(csr, "eid", g, None, "sum", 0, None)
        else:
            gx, _ = _aggregate_any(csr, "eid", g, "sum", 0)
        return gx, None


_range_cache = _Cache()


def index_range(idx):
    """(min, max) of an index tensor: one aminmax and one host read the first
    time, then cached on the tensor (identity + version counter + data pointer,
    dropped with it -- graph._Cache), so the per-forward checks of a reused
    edge_index cost a dictionary lookup, not a device sync.

    Limitation (the same contract as the per-edge_index CSR cache, graph_for):
    a write that does not bump the version counter -- through ``.data``, a
    DLPack / from_blob alias, or a raw-pointer kernel -- is not seen.  After such
    a write call forget_index(idx) (or mutate through ordinary in-place ops)."""
    def compute():
        mn, mx = torch.aminmax(idx)
        return tuple(torch.stack([mn, mx]).tolist())
    return _range_cache.get(idx, ("range", idx.data_ptr()), compute)


def forget_index(idx):
    """Drop every cached fact about idx (its range and CSR graphs): for index
    tensors written behind autograd's back (see index_range)."""
    from .graph import _graph_cache, _index_cache, _key_cache
    base = idx._base if idx._base is not None else idx
    for c in (_range_cache, _graph_cache, _index_cache, _key_cache):
        c._drop(id(base))


def check_row_index(idx, n, what="index_select"):
    """IndexError when an index falls outside [0, n), as x.index_select(0, idx)
    raises on the CPU (the native row gather reads whatever row it is given, so
    a bad index must never reach it).  The range is cached per index tensor
    (index_range); skipped while a HIP graph is being captured (the captured
    call was checked when it ran eagerly before capture, and a capture cannot
    read values back)."""
    if idx.numel() == 0 or (idx.is_cuda and torch.cuda.is_current_stream_capturing()):
        return
    lo, hi = index_range(idx)
    if lo < 0 or hi >= n:
        raise IndexError("%s: index %d out of range for %d rows" % (what, lo if lo < 0 else hi, n))


def index_select_rows(x, idx):
    """Differentiable native replacement of x.index_select(0, idx) for 2-D x
    (fp32 / fp64 / fp16 / bf16 / int64); an index outside [0, x.size(0))
    raises IndexError (check_row_index)."""
    _lib.require_device(x, idx)
    x = _any_2d(x, "x")
    check_row_index(idx, x.shape[0])
    return GatherRows.apply(x, idx)


# ---------------------------------------------------------------------------
# self-loop rewrites (PyG 1.4.3 utils.loop [U4])
# ---------------------------------------------------------------------------

_LOOP_MODES = {"remove": _lib.MP_LOOPS_REMOVE, "add": _lib.MP_LOOPS_ADD,
               "add_remaining": _lib.MP_LOOPS_ADD_REMAINING}


def self_loops(edge_index, num_nodes, mode):
    """Native loop rewrite of a [2, E] int64 device edge_index (mp_self_loops).

    Returns (edge_index_out, pos): the kept edges in original order, then (for
    'add' / 'add_remaining') the loops 0..N-1; pos[k] = input position whose
    weight output edge k carries (-1: fill value).  One host sync reads the
    number of self loops (the output size), like upstream's boolean-mask
    indexing."""
    _lib.require_device(edge_index)
    nat = _lib.native()
    dev = edge_index.device
    st = _lib.stream_ptr(dev)
    N = int(num_nodes)
    E = int(edge_index.shape[1])
    row = edge_index[0].to(torch.int64).contiguous()
    col = edge_index[1].to(torch.int64).contiguous()
    m = _LOOP_MODES[mode]
    n_kept = E
    if m != _lib.MP_LOOPS_ADD and E:
        cnt = torch.empty(2, dtype=torch.int64, device=dev)
        nat.mp_self_loop_count(row.data_ptr(), col.data_ptr(), E, N, cnt.data_ptr(), st)
        n_loops, n_bad = cnt.tolist()
        if n_bad and m == _lib.MP_LOOPS_ADD_REMAINING:
            # upstream: loop_weight[row[inv_mask]] = ... raises for these
            raise IndexError("mi355_mp: %d self loops name a node outside [0, %d)" % (n_bad, N))
        n_kept = E - n_loops
    n_out = n_kept + (0 if m == _lib.MP_LOOPS_REMOVE else N)
    out = torch.empty((2, n_out), dtype=torch.int64, device=dev)
    pos = torch.empty(max(n_out, 1), dtype=torch.int64, device=dev)
    wsb = nat.mp_self_loops_workspace(E, N)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    nat.mp_self_loops(row.data_ptr(), col.data_ptr(), E, N, m, n_kept, out[0].data_ptr(), out[1].data_ptr(),
                      pos.data_ptr(), ws.data_ptr(), wsb, st)
    return out, pos[:n_out]


class _GatherFill(torch.autograd.Function):
    """out[k] = w[pos[k]] if pos[k] >= 0 else fill (native); every input
    position appears at most once in pos, so the backward is a plain scatter."""

    @staticmethod
    def forward(ctx, w, pos, fill):
        ctx.n = w.shape[0]
        ctx.save_for_backward(pos)
        out = torch.empty(pos.shape[0], dtype=torch.float32, device=w.device)
        _lib.native().mp_gather_fill_f32(w.data_ptr(), pos.data_ptr(), pos.shape[0], float(fill), out.data_ptr(),
                                         _lib.stream_ptr(w.device))
        return out

    @staticmethod
    def backward(ctx, g):
        (pos,) = ctx.saved_tensors
        keep = pos >= 0
        gw = torch.zeros(ctx.n, dtype=g.dtype, device=g.device)
        gw[pos[keep]] = g[keep]
        return gw, None, None


def gather_fill(w, pos, fill):
    """Per-edge weights of a loop rewrite: w[pos] with `fill` where pos < 0."""
    _lib.require_device(w, pos)
    if w.dtype != torch.float32:
        v = w[pos.clamp(min=0)]
        return torch.where(pos >= 0, v, torch.full_like(v, fill))
    return _GatherFill.apply(w.contiguous(), pos, fill)


# ---------------------------------------------------------------------------
# GCN normalisation (GCNConv.norm [U5])
# ---------------------------------------------------------------------------

def segment_sum_serial(csr, values, out=None):
    """out[r] = sum over the slots of row r, in slot order, of values[eid[k]]
    (mp_segment_sum_serial_f32): a 1-D scatter_add_ in the reference's edge
    order, bit for bit (csr keyed on the scatter index; values in original
    edge order, fp32)."""
    _lib.require_device(values)
    v = values.to(torch.float32).contiguous()
    if out is None:
        out = torch.empty(max(csr.n_rows, 1), dtype=torch.float32, device=v.device)[:csr.n_rows]
    _lib.native().mp_segment_sum_serial_f32(csr.rowptr.data_ptr(), csr.eid.data_ptr(), v.data_ptr(), csr.n_rows,
                                            out.data_ptr(), _lib.stream_ptr(v.device))
    return out


def norm_from_degree(row, col, deg, edge_weight, trusted=False):
    """dinv = deg^-1/2 (inf -> 0, torch's CPU pow(-0.5) rounding), then
    dinv[row] * w * dinv[col] (mp_gcn_norm_from_deg_f32).  deg is consumed.
    The kernel reads deg[row[e]] and deg[col[e]]: an id outside [0, deg.numel())
    raises IndexError first, as the reference's deg_inv_sqrt[row] / [col] does.
    trusted=True (ids the caller built in range, e.g. a shard plan's local
    edges): no range check, so no host read-back."""
    _lib.require_device(row, col, deg, edge_weight)
    if not trusted:
        check_row_index(row, deg.numel(), "gcn_norm (row)")
        check_row_index(col, deg.numel(), "gcn_norm (col)")
    E = row.numel()
    w = edge_weight.to(torch.float32).contiguous() if edge_weight is not None else None
    norm = torch.empty(E, dtype=torch.float32, device=row.device)
    d = deg.to(torch.float32).contiguous()
    row, col = row.contiguous(), col.contiguous()  # named: a temporary copy could be freed before the launch
    _lib.native().mp_gcn_norm_from_deg_f32(row.data_ptr(), col.data_ptr(), _lib.ptr(w), E, d.numel(), d.data_ptr(),
                                           norm.data_ptr(), _lib.stream_ptr(row.device))
    return norm


def gcn_norm_weights(edge_index, num_nodes, edge_weight=None, integer_weights=False):
    """norm[e] = deg^-1/2[row] * w[e] * deg^-1/2[col], deg = scatter_add(w, row).

    edge_index must already carry the self loops (add_remaining_self_loops).
    integer_weights: the caller guarantees integer-valued weights (GCNConv's
    structure-only norm: ones and the loop fill 1 / 2): the degree is then
    exact in any order and mp_gcn_norm_f32 sums it with atomics.  Otherwise the
    degree is the transposed CSR's serial segment sum
    (mp_segment_sum_serial_f32): the reference's edge-order sum bit for bit,
    deterministic; that CSR is the one the layer's backward uses anyway.
    """
    _lib.require_device(edge_index, edge_weight)
    nat = _lib.native()
    E = edge_index.shape[1]
    N = int(num_nodes)
    # the degree kernel adds at deg[row[e]]: a node id outside [0, N) raises
    # here, as the reference's scatter_add(edge_weight, row, dim_size=N) does
    check_row_index(edge_index, N, "gcn_norm")
    dev = edge_index.device
    st = _lib.stream_ptr(dev)
    row = edge_index[0].contiguous()
    col = edge_index[1].contiguous()
    w = edge_weight.to(torch.float32).contiguous() if edge_weight is not None else None
    deg = torch.empty(max(N, 1), dtype=torch.float32, device=dev)
    norm = torch.empty(E, dtype=torch.float32, device=dev)
    if w is None or integer_weights or E == 0:
        nat.mp_gcn_norm_f32(row.data_ptr(), col.data_ptr(), _lib.ptr(w), E, N, deg.data_ptr(), norm.data_ptr(), st)
        return norm
    from .graph import graph_for
    rows = graph_for(edge_index, N, N, "source_to_target").src   # CSR keyed on edge_index[0]
    segment_sum_serial(rows, w, out=deg[:N])
    nat.mp_gcn_norm_from_deg_f32(row.data_ptr(), col.data_ptr(), w.data_ptr(), E, N, deg.data_ptr(), norm.data_ptr(),
                                 st)
    return norm


# ---------------------------------------------------------------------------
# GATConv fused attention aggregation (GATConv.message + utils.softmax [U3,U6])
# ---------------------------------------------------------------------------

# GAT forward form.  Default: one online-softmax pass (mp_gat_aggregate_f32).
# GAT_TWO_PASS = True selects mp_gat_softmax_aggregate_f32, which follows the
# reference's operation order (softmax row max, then the denominator summed in
# edge order, then alpha * x_j summed in edge order) at a cost: on config 3 its
# two statistics passes take 3.6 ms and its 64-feature-tile aggregation 10.6 ms
# (one a_src gather per slot per tile), against 8.6 ms for the single pass
# (DESIGN.md section 3.3).
GAT_TWO_PASS = False
# The single pass recomputes a_src[j] from each gathered xw row (bitwise the
# node-score kernel's value) instead of gathering it: mp_gat_aggregate_att_f32.
GAT_OWN_A_SRC = True


def gat_two_pass(csr, H, C):
    return GAT_TWO_PASS and bool(_lib.native().mp_gat_two_pass_ok(H, C))


# Training forward: the fused pass also leaves sum_j alpha leaky' xw_j and
# sum_j alpha leaky' per (row, head) (mp_gat_aggregate_train_f32), which make the
# backward's d a_dst node-wise: no per-edge d score array, no segmented pass.
GAT_TRAIN_FWD = True
# The fused forward computes each row's node scores (a_src, a_dst) from the
# row's own xw (mp_gat_forward_f32 / mp_gat_forward_train_f32, bitwise the
# node-score kernel's values) instead of running mp_gat_node_scores_f32 first.
# Config 3 (inference): main 7.78 ms, no 0.50 ms node-score pass -> 7.85 vs 8.30 ms.
GAT_NODE_SCORES_IN_KERNEL = os.environ.get("MP_GAT_ND", "1") != "0"   # MP_GAT_ND=0: A/B runs
# The training forward with in-kernel scores needs 92 VGPRs (5 waves / SIMD
# instead of 6): GATConv forward + backward 26.49 vs 26.28 ms on config 3, so
# training keeps the separate node-score pass (MP_GAT_ND_TRAIN=1 selects it).
GAT_NODE_SCORES_IN_KERNEL_TRAIN = os.environ.get("MP_GAT_ND_TRAIN", "0") == "1"


def _gat_nd_ok(graph, xw, H, C, bias):
    return (GAT_NODE_SCORES_IN_KERNEL and GAT_OWN_A_SRC and bool(_lib.native().mp_gat_train_ok(H, C))
            and not gat_two_pass(graph.dst, H, C) and xw.data_ptr() % 16 == 0 and graph.n_dst == xw.shape[0]
            and graph.n_src == xw.shape[0] and (bias is None or bias.data_ptr() % 16 == 0))


def _gat_train_fwd_ok(graph, xw, H, C):
    """The training forward (mp_gat_aggregate_train_f32) applies: C % 4 == 0
    (a_src from the gathered rows when C/4 is a power of two <= 64, else from
    the node-score array)."""
    return (GAT_TRAIN_FWD and GAT_OWN_A_SRC and gat_wide_ok(H, C)
            and not gat_two_pass(graph.dst, H, C) and xw.data_ptr() % 16 == 0 and _gat_rows_ok(graph, xw))


def _gat_rows_ok(graph, xw):
    """The fused GAT kernels take a square graph (n_dst == n_src == xw rows) or a
    sharded rank's local graph: n_src == xw rows and destination row i's own xw
    row is row i of xw (the rank's own rows first, then its halo rows:
    mi355_mp.dist.ShardedGraph.gat_propagate), so n_dst <= n_src."""
    return graph.n_src == xw.shape[0] and graph.n_dst <= xw.shape[0]


def _pad_rows(t, n):
    """t [m, ...] -> [n, ...] with zero rows appended (node-wise gradients of the
    destination rows, extended over the halo rows of a sharded local graph)."""
    if t.shape[0] == n:
        return t
    out = t.new_zeros((n,) + tuple(t.shape[1:]))
    out[:t.shape[0]] = t
    return out


def gat_wide_ok(H, C):
    """Heads of any width with C % 4 == 0 (GATConv pads C to it): the fused
    training forward reads a_src from the node-score array when C/4 is not a
    power of two <= 64, and the backward runs the wide form (mp_gat_backward_wide_f32)."""
    return bool(_lib.native().mp_gat_wide_ok(H, C))


def gat_dropout_ok(H, C, p):
    """The fused path carries GATConv's attention dropout (training, 0 < p < 1):
    the training forward and its transposed backward evaluate one hashed keep
    mask per (edge, head) (mp_gat_aggregate_train_drop_f32; the edge's key is
    its id -- the global id on a shard: Graph.drop_ids)."""
    return (0.0 < float(p) < 1.0 and GAT_TRAIN_FWD and GAT_OWN_A_SRC and 1 <= H <= 32 and gat_wide_ok(H, C))


def gat_dropout_keep(graph, seed, p, H):
    """The attention-dropout keep mask [E, H] (bool, the graph's edge order) that
    the fused GAT kernels apply for (seed, p): mp_gat_dropout_keep over the
    destination-CSR slots with their keys (Graph.drop_ids), mapped back through
    the CSR's edge ids."""
    nat = _lib.native()
    csr = graph.dst
    E = csr.n_edges
    dev = csr.rowptr.device
    bits = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    nat.mp_gat_dropout_keep(int(seed) & 0xFFFFFFFFFFFFFFFF, float(p), int(H), E, graph.drop_ids("dst").data_ptr(),
                            bits.data_ptr(), _lib.stream_ptr(dev))
    shifts = torch.arange(H, dtype=torch.int32, device=dev)
    keep_slot = ((bits[:E].unsqueeze(1) >> shifts) & 1).bool()
    keep = torch.empty_like(keep_slot)
    keep[csr.eid[:E].long()] = keep_slot
    return keep


def _gat_forward(graph, edge_index, xw, att, H, C, slope, bias, want_alpha, train2=False, drop=None):
    """Returns (out, alpha, a_src, a_dst, stats, extra).  train2 (callers check
    _gat_train_fwd_ok first): the training forward, out = aggregate + bias and
    extra = (agg2, s2); else extra = None.  No pre-bias copy of the aggregate
    is written: the backward prologues take rs over out - bias (ABI 6).
    drop = (seed, p): attention dropout on the messages (train2 only)."""
    nat = _lib.native()
    dev = xw.device
    N = xw.shape[0]
    csr = graph.dst
    st = _lib.stream_ptr(dev)
    if not _gat_rows_ok(graph, xw):
        raise ValueError("mi355_mp: fused GAT needs n_src == x.size(0) >= n_dst (a square graph, or a sharded "
                         "rank's own rows followed by its halo rows)")
    att_c = att.reshape(H, 2 * C).contiguous().to(torch.float32)
    a_src = torch.empty((N, H), dtype=torch.float32, device=dev)
    a_dst = torch.empty((N, H), dtype=torch.float32, device=dev)
    if drop is not None and not train2:
        raise ValueError("mi355_mp: fused attention dropout runs in the training forward only")
    nd = (_gat_nd_ok(graph, xw, H, C, bias) and (GAT_NODE_SCORES_IN_KERNEL_TRAIN or not train2)
          and drop is None)
    if N and not nd:
        nat.mp_gat_node_scores_f32(xw.data_ptr(), N, H, C, att_c.data_ptr(), a_src.data_ptr(), a_dst.data_ptr(), st)
    out = torch.empty((graph.n_dst, H * C), dtype=torch.float32, device=dev)
    stats = torch.empty((graph.n_dst, H, 2), dtype=torch.float32, device=dev)
    g = csr.struct("other")
    extra = None
    if train2 and nd:
        agg2 = torch.empty((graph.n_dst, H * C), dtype=torch.float32, device=dev)
        s2 = torch.empty((graph.n_dst, H), dtype=torch.float32, device=dev)
        sb = nat.mp_gat_train_slab_bytes(g, H, C)
        slab = torch.empty(sb, dtype=torch.uint8, device=dev)
        nat.mp_gat_forward_train_f32(g, xw.data_ptr(), att_c.data_ptr(), H, C, float(slope), _lib.ptr(bias),
                                     out.data_ptr(), out.stride(0), None, stats.data_ptr(), agg2.data_ptr(),
                                     s2.data_ptr(), a_src.data_ptr(), a_dst.data_ptr(), slab.data_ptr(), sb,
                                     _lib.MP_STAGE_ALL, st)
        extra = (agg2, s2)
    elif train2:
        agg2 = torch.empty((graph.n_dst, H * C), dtype=torch.float32, device=dev)
        s2 = torch.empty((graph.n_dst, H), dtype=torch.float32, device=dev)
        sb = nat.mp_gat_train_slab_bytes(g, H, C)
        slab = torch.empty(sb, dtype=torch.uint8, device=dev)
        if drop is not None:
            nat.mp_gat_aggregate_train_drop_f32(g, xw.data_ptr(), a_src.data_ptr(), a_dst.data_ptr(), att_c.data_ptr(),
                                                H, C, float(slope), _lib.ptr(bias), out.data_ptr(), out.stride(0), None,
                                                stats.data_ptr(), agg2.data_ptr(), s2.data_ptr(), int(drop[0]),
                                                float(drop[1]), graph.drop_ids("dst").data_ptr(), slab.data_ptr(), sb,
                                                _lib.MP_STAGE_ALL, st)
        else:
            nat.mp_gat_aggregate_train_f32(g, xw.data_ptr(), a_src.data_ptr(), a_dst.data_ptr(), att_c.data_ptr(), H, C,
                                           float(slope), _lib.ptr(bias), out.data_ptr(), out.stride(0), None,
                                           stats.data_ptr(), agg2.data_ptr(), s2.data_ptr(), slab.data_ptr(), sb,
                                           _lib.MP_STAGE_ALL, st)
        extra = (agg2, s2)
    if extra is None:
        sb = nat.mp_gat_slab_bytes(g, H, C)
        slab = torch.empty(sb, dtype=torch.uint8, device=dev)
        if nd:
            nat.mp_gat_forward_f32(g, xw.data_ptr(), att_c.data_ptr(), H, C, float(slope), _lib.ptr(bias),
                                   out.data_ptr(), out.stride(0), a_src.data_ptr(), a_dst.data_ptr(), stats.data_ptr(),
                                   slab.data_ptr(), sb, _lib.MP_STAGE_ALL, st)
        elif gat_two_pass(csr, H, C):
            nat.mp_gat_softmax_aggregate_f32(g, csr.slot_rows().data_ptr(), xw.data_ptr(), a_src.data_ptr(),
                                             a_dst.data_ptr(), H, C, float(slope), _lib.ptr(bias), out.data_ptr(),
                                             out.stride(0), stats.data_ptr(), slab.data_ptr(), sb, _lib.MP_STAGE_ALL,
                                             st)
        else:
            nat.mp_gat_aggregate_att_f32(g, xw.data_ptr(), a_src.data_ptr(), a_dst.data_ptr(),
                                         att_c.data_ptr() if GAT_OWN_A_SRC else None, H, C, float(slope),
                                         _lib.ptr(bias), out.data_ptr(), out.stride(0), stats.data_ptr(),
                                         slab.data_ptr(), sb, _lib.MP_STAGE_ALL, st)
    alpha = None
    if want_alpha:
        E = edge_index.shape[1]
        alpha = torch.empty((E, H), dtype=torch.float32, device=dev)
        src = edge_index[graph.j].contiguous()
        dst = edge_index[graph.i].contiguous()
        nat.mp_gat_alpha_f32(src.data_ptr(), dst.data_ptr(), E, H, a_src.data_ptr(), a_dst.data_ptr(), float(slope),
                             stats.data_ptr(), alpha.data_ptr(), st)
    return out, alpha, a_src, a_dst, stats, extra


def _heads_aggregate(csr, gather, w_slot, H, x):
    """out[r, h*C+c] = sum_k w_slot[k, h] * x[col_k, h*C+c] (mp_aggregate_heads_f32)."""
    nat = _lib.native()
    F = x.shape[1]
    out = torch.empty((csr.n_rows, F), dtype=torch.float32, device=x.device)
    if csr.n_rows == 0:
        return out
    g = csr.struct(gather)
    sb = nat.mp_aggregate_slab_bytes(g, F, 0)
    slab = torch.empty(sb, dtype=torch.uint8, device=x.device)
    nat.mp_aggregate_heads_f32(g, w_slot.data_ptr(), H, x.data_ptr(), x.stride(0), F, out.data_ptr(), out.stride(0),
                               slab.data_ptr(), sb, _lib.MP_STAGE_ALL, _lib.stream_ptr(x.device))
    return out


def _gat_bwd_fused_ok(C):
    """mp_gat_backward_f32 reduces a head's dot product over C/4 (or C) lanes."""
    def pow2(q):
        return 1 <= q <= 64 and (q & (q - 1)) == 0
    return (C % 4 == 0 and pow2(C // 4)) or pow2(C)


def _gat_backward_wide(graph, g, xw, att, a_src, a_dst, stats, agg, agg_bias, extra, H, C, slope, want_att,
                       want_bias, drop=None):
    """GATConv backward for heads of any width (C % 4 == 0), after the training
    forward: prep (pack + node-wise d a_dst), one pass over the transposed CSR
    with no per-slot dot product (mp_gat_backward_wide_f32: sum alpha g_i,
    sum lk alpha g_i, sum lk alpha rs_i per source row), then the node-wise
    epilogue (d a_src = <acc2, xw> - sc, the att terms of d xw).  agg: the
    forward's output, agg_bias the bias inside it (None: none).
    Returns (d xw, d att or None, d bias or None)."""
    nat = _lib.native()
    dev = xw.device
    st = _lib.stream_ptr(dev)
    N = xw.shape[0]
    F = H * C
    att_c = att.reshape(H, 2 * C).contiguous()
    if N == 0:
        return (torch.zeros_like(xw), torch.zeros_like(att) if want_att else None,
                g.new_zeros(F) if want_bias else None)
    agg2, s2 = extra
    n_dst = graph.n_dst            # < N on a sharded rank's local graph (halo rows receive no edges)
    pack = torch.empty((max(n_dst, 1), H, 4), dtype=torch.float32, device=dev)
    ga_dst = (torch.empty if n_dst == N else torch.zeros)((N, H), dtype=torch.float32, device=dev)
    if n_dst:
        nat.mp_gat_backward_prep_wide_f32(g.data_ptr(), g.stride(0), agg.data_ptr(), agg.stride(0), _lib.ptr(agg_bias),
                                          agg2.data_ptr(), s2.data_ptr(), a_dst.data_ptr(), stats.data_ptr(), n_dst, H,
                                          C, pack.data_ptr(), _lib.nbytes(pack), ga_dst.data_ptr(), st)
    src = graph.src_with_dst_slots()
    gs = src.struct("dst_slot")
    gx = torch.empty((N, F), dtype=torch.float32, device=dev)
    acc2 = torch.empty((N, F), dtype=torch.float32, device=dev)
    sc = torch.empty((N, H), dtype=torch.float32, device=dev)
    sb = nat.mp_gat_train_slab_bytes(gs, H, C)
    slab = torch.empty(sb, dtype=torch.uint8, device=dev)
    seed, p = (0, 0.0) if drop is None else (int(drop[0]), float(drop[1]))
    ids = graph.drop_ids("src").data_ptr() if drop is not None else None
    nat.mp_gat_backward_wide_f32(gs, g.data_ptr(), g.stride(0), a_src.data_ptr(), pack.data_ptr(), H, C, float(slope),
                                 seed, p, ids, gx.data_ptr(), acc2.data_ptr(), _lib.nbytes(acc2), sc.data_ptr(),
                                 _lib.nbytes(sc), slab.data_ptr(), sb, _lib.MP_STAGE_ALL, st)
    del slab, pack
    nat.mp_gat_backward_epilogue_wide_f32(gx.data_ptr(), acc2.data_ptr(), xw.data_ptr(), att_c.data_ptr(),
                                          ga_dst.data_ptr(), sc.data_ptr(), N, H, C, st)
    del acc2
    ga_src = sc
    gatt = None
    if want_att:
        x3 = xw.view(N, H, C)
        gatt = torch.cat([torch.einsum("nh,nhc->hc", ga_dst, x3), torch.einsum("nh,nhc->hc", ga_src, x3)],
                         dim=-1).view_as(att)
    gb = col_sums(g) if want_bias else None
    return gx, gatt, gb


def _att_part_blocks(n_rows, n_dst):
    """Blocks of the d att partials of mp_gat_backward_finish_f32: the pass runs
    over all n_rows rows of xw (own + halo rows on a sharded rank's local graph,
    n_dst of them own), one partial per block of mp_gat_bwd_blocks(n_rows).
    (Round 4 sized this for n_dst: the library now rejects such a buffer --
    ABI 6 extents -- instead of writing past it; tests/test_gpu_dist.py.)"""
    return int(_lib.native().mp_gat_bwd_blocks(n_rows))


def _gat_backward_fused(graph, g, xw, att, a_src, a_dst, stats, agg, agg_bias, H, C, slope, want_att, want_bias,
                        extra=None, drop=None):
    """GATConv backward: prep (packed destination terms + bias-grad partials),
    one gather pass over the transposed CSR (mp_gat_backward_f32), the d a_dst
    row sums over the dst CSR (reading the per-edge d score through the
    src-slot map), and the epilogue (att_dst term + att-grad partials).  agg:
    the forward's output, agg_bias the bias inside it (None: none).
    Returns (d xw, d att or None, d bias or None)."""
    nat = _lib.native()
    dev = xw.device
    st = _lib.stream_ptr(dev)
    N = xw.shape[0]
    F = H * C
    att_c = att.reshape(H, 2 * C).contiguous()
    if N == 0:
        return (torch.zeros_like(xw), torch.zeros_like(att) if want_att else None,
                g.new_zeros(F) if want_bias else None)
    epi = C % 4 == 0 and F <= 256
    n_dst = graph.n_dst            # < N on a sharded rank's local graph (halo rows receive no edges)
    nb = int(nat.mp_gat_bwd_blocks(n_dst))
    pack = torch.empty((max(n_dst, 1), H, 4), dtype=torch.float32, device=dev)
    gpart = torch.empty((nb, F), dtype=torch.float32, device=dev) if (want_bias and epi and n_dst) else None
    ga_dst = None
    if extra is not None:
        # d a_dst[n,h] = <g_n, agg2_n>_h - rs_n,h s2_n,h: node-wise, no per-edge d score
        agg2, s2 = extra
        ga_dst = (torch.empty if n_dst == N else torch.zeros)((N, H), dtype=torch.float32, device=dev)
        if n_dst:
            nat.mp_gat_backward_prep_train_f32(g.data_ptr(), g.stride(0), agg.data_ptr(), agg.stride(0),
                                               _lib.ptr(agg_bias), agg2.data_ptr(), s2.data_ptr(), a_dst.data_ptr(),
                                               stats.data_ptr(), n_dst, H, C, pack.data_ptr(), _lib.nbytes(pack),
                                               _lib.ptr(gpart), _lib.nbytes(gpart), ga_dst.data_ptr(), st)
    elif n_dst:
        nat.mp_gat_backward_prep_f32(g.data_ptr(), g.stride(0), agg.data_ptr(), agg.stride(0), _lib.ptr(agg_bias),
                                     a_dst.data_ptr(), stats.data_ptr(), n_dst, H, C, pack.data_ptr(),
                                     _lib.nbytes(pack), _lib.ptr(gpart), _lib.nbytes(gpart), st)
    gb = None
    if want_bias:
        gb = gpart.sum(0) if gpart is not None else g.sum(0)
    src = graph.src_with_dst_slots()
    E = src.n_edges
    gx = torch.empty((N, F), dtype=torch.float32, device=dev)
    ga_src = torch.empty((N, H), dtype=torch.float32, device=dev)
    # per-edge d score in dst-CSR slot order (only without the training forward's extras)
    de = torch.empty((max(E, 1), H), dtype=torch.float32, device=dev) if ga_dst is None else None
    gs = src.struct("dst_slot")
    sb = nat.mp_gat_slab_bytes(gs, H, C)
    slab = torch.empty(sb, dtype=torch.uint8, device=dev)
    fused_dst = ga_dst is not None
    if drop is not None:
        if not fused_dst:
            raise ValueError("mi355_mp: the attention-dropout backward needs the training forward's extras")
        nat.mp_gat_backward_train_drop_f32(gs, g.data_ptr(), g.stride(0), xw.data_ptr(), a_src.data_ptr(),
                                           pack.data_ptr(), att_c.data_ptr(), H, C, float(slope), ga_dst.data_ptr(),
                                           int(drop[0]), float(drop[1]), graph.drop_ids("src").data_ptr(),
                                           gx.data_ptr(), ga_src.data_ptr(), slab.data_ptr(), sb, _lib.MP_STAGE_ALL, st)
    elif fused_dst:
        # the transposed pass also adds d a_dst (x) att_dst to each row's d xw
        nat.mp_gat_backward_train_f32(gs, g.data_ptr(), g.stride(0), xw.data_ptr(), a_src.data_ptr(), pack.data_ptr(),
                                      att_c.data_ptr(), H, C, float(slope), ga_dst.data_ptr(), gx.data_ptr(),
                                      ga_src.data_ptr(), slab.data_ptr(), sb, _lib.MP_STAGE_ALL, st)
    else:
        nat.mp_gat_backward_f32(gs, g.data_ptr(), g.stride(0), xw.data_ptr(), a_src.data_ptr(), pack.data_ptr(),
                                att_c.data_ptr(), H, C, float(slope), gx.data_ptr(), ga_src.data_ptr(), _lib.ptr(de),
                                _lib.nbytes(de), slab.data_ptr(), sb, _lib.MP_STAGE_ALL, st)
    del slab, pack
    if ga_dst is None:
        ga_dst, _ = _aggregate(graph.dst, "slot", de, None, "sum", 0, None)
        ga_dst = _pad_rows(ga_dst, N)
        del de
    gatt = None
    if epi:
        if want_att or not fused_dst:
            # att_dst term of d xw (unless the transposed pass added it) + d att partials:
            # the finish pass runs over all N rows (own + halo on a sharded rank's
            # local graph), one partial per block of mp_gat_bwd_blocks(N)
            apart = torch.empty((_att_part_blocks(N, n_dst), 2, F), dtype=torch.float32, device=dev)
            nat.mp_gat_backward_finish_f32(None if fused_dst else gx.data_ptr(), xw.data_ptr(), ga_dst.data_ptr(),
                                           ga_src.data_ptr(), att_c.data_ptr(), N, H, C, apart.data_ptr(),
                                           _lib.nbytes(apart), st)
        if want_att:
            p = apart.sum(0).view(2, H, C)
            gatt = torch.cat([p[0], p[1]], dim=-1).view_as(att)
    else:
        if not fused_dst:
            nat.mp_heads_outer_add_f32(gx.data_ptr(), gx.stride(0), ga_dst.data_ptr(), N, H, C, att_c.data_ptr(), 2 * C,
                                       st)
        if want_att:
            x3 = xw.view(N, H, C)
            gatt = torch.cat([torch.einsum("nh,nhc->hc", ga_dst, x3), torch.einsum("nh,nhc->hc", ga_src, x3)],
                             dim=-1).view_as(att)
    return gx, gatt, gb


class _GatPropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xw, att, bias, graph, edge_index, H, C, slope, want_alpha, train, drop=None):
        # attention dropout (drop = (seed, p)) runs in the training forward, with
        # or without a backward to follow (training mode under no_grad)
        wide = not _gat_bwd_fused_ok(C) and gat_wide_ok(H, C)
        fused = (train or drop is not None) and (_gat_bwd_fused_ok(C) or wide)
        # the fused backward's rs_i = <g_i, agg_i> comes from the saved output
        # (agg + bias, bias fused into the forward) and the bias: the prologue
        # takes rs over out - bias, so no pre-bias copy is written (ABI 6).  The
        # output is saved, so an in-place change of it before backward raises
        # torch's usual "modified by an inplace operation" error.
        train2 = fused and _gat_train_fwd_ok(graph, xw, H, C)
        if wide and fused and not train2:
            fused = False  # the wide backward needs the training forward's extras
        if drop is not None and not train2:
            raise ValueError("mi355_mp: fused attention dropout needs the training forward (gat_dropout_ok)")
        out, alpha, a_src, a_dst, stats, extra = _gat_forward(graph, edge_index, xw, att, H, C, slope, bias,
                                                              want_alpha, train2=train2, drop=drop)
        ctx.graph, ctx.H, ctx.C, ctx.slope, ctx.drop = graph, H, C, slope, drop
        ctx.wide = wide
        ctx.has_bias = bias is not None
        ctx.fused = fused
        ctx.has_extra = extra is not None
        ctx.save_for_backward(xw, att, edge_index, a_src, a_dst, stats, out if fused else None,
                              bias if fused else None, *(extra if extra is not None else ()))
        if alpha is not None:
            ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    def backward(ctx, grad_out, _ga=None):
        """Native GAT backward over the two CSRs of the graph:
          dx_j   = sum_i alpha_ij g_i          (per-head weighted transposed aggregation)
          dalpha = <g_i, xw_j> per head        (CSR SDDMM)
          ds     = alpha (dalpha - sum_row alpha dalpha)   (softmax backward)
          de     = ds * leaky'(s);  d a_dst = row sums, d a_src = column sums of de
          dxw   += d a_src (x) att_src + d a_dst (x) att_dst;  d att = sum_n d a (x) xw
        Only [E, H]-sized arrays are materialised, never [E, H*C]."""
        nat = _lib.native()
        xw, att, edge_index, a_src, a_dst, stats, agg, agg_bias = ctx.saved_tensors[:8]
        extra = tuple(ctx.saved_tensors[8:10]) if ctx.has_extra else None
        graph, H, C, slope = ctx.graph, ctx.H, ctx.C, ctx.slope
        dev = xw.device
        st = _lib.stream_ptr(dev)
        g = grad_out.contiguous()
        if g.data_ptr() % 16:
            g = g.clone()  # a view at an odd offset: the 4-wide transposed pass (the dropout form has no other) needs 16-B rows
        N = xw.shape[0]
        if ctx.fused and ctx.wide:
            gx, gatt, gb = _gat_backward_wide(graph, g, xw, att, a_src, a_dst, stats, agg, agg_bias, extra, H, C,
                                              slope, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2],
                                              ctx.drop)
            return gx, gatt, gb, None, None, None, None, None, None, None, None
        if ctx.fused:
            gx, gatt, gb = _gat_backward_fused(graph, g, xw, att, a_src, a_dst, stats, agg, agg_bias, H, C, slope,
                                               ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2],
                                               extra, ctx.drop)
            return gx, gatt, gb, None, None, None, None, None, None, None, None
        gb = col_sums(g) if ctx.has_bias and ctx.needs_input_grad[2] else None
        dst, src = graph.dst, graph.src
        E = dst.n_edges
        sr = dst.slot_rows()
        alpha = torch.empty((max(E, 1), H), dtype=torch.float32, device=dev)
        score = torch.empty_like(alpha)
        nat.mp_gat_alpha_csr_f32(dst.struct("other"), sr.data_ptr(), a_src.data_ptr(), a_dst.data_ptr(), H,
                                 float(slope), stats.data_ptr(), alpha.data_ptr(), score.data_ptr(), st)
        eid_d = dst.eid[:E].long()
        # message part of d xw: alpha in the transposed CSR's slot order
        alpha_orig = torch.empty_like(alpha)
        alpha_orig[eid_d] = alpha
        alpha_src = alpha_orig[src.eid[:E].long()].contiguous()
        gx = _heads_aggregate(src, "other", alpha_src, H, g)
        # d alpha (CSR order) and the softmax backward
        dalpha = torch.empty_like(alpha)
        nat.mp_gat_sddmm_f32(dst.struct("other"), sr.data_ptr(), g.data_ptr(), g.stride(0), xw.data_ptr(), xw.stride(0),
                             H, C, dalpha.data_ptr(), st)
        t = (alpha * dalpha)[:E].contiguous()
        rs, _ = _aggregate(dst, "slot", t, None, "sum", 0, None)             # sum over each row's slots
        ds = alpha[:E] * (dalpha[:E] - rs[sr[:E].long()])
        de = (ds * torch.where(score[:E] > 0, torch.ones_like(ds), torch.full_like(ds, slope))).contiguous()
        ga_dst, _ = _aggregate(dst, "slot", de, None, "sum", 0, None)
        ga_dst = _pad_rows(ga_dst, N)
        de_orig = torch.empty_like(de)
        de_orig[eid_d] = de
        ga_src, _ = _aggregate(src, "eid", de_orig, None, "sum", 0, None)
        att3 = att.reshape(H, 2 * C)
        x3 = xw.view(N, H, C)
        gx = gx.view(N, H, C) + ga_src.unsqueeze(-1) * att3[:, C:].unsqueeze(0) \
            + ga_dst.unsqueeze(-1) * att3[:, :C].unsqueeze(0)
        gatt = None
        if ctx.needs_input_grad[1]:
            gd = torch.einsum("nh,nhc->hc", ga_dst, x3)
            gs = torch.einsum("nh,nhc->hc", ga_src, x3)
            gatt = torch.cat([gd, gs], dim=-1).view_as(att)
        return gx.reshape(N, H * C), gatt, gb, None, None, None, None, None, None, None, None


_MASK64 = 0xFFFFFFFFFFFFFFFF
_seed_calls = {}


def _mix64(z):
    """splitmix64 finaliser: spreads (seed, offset) pairs over the 64-bit keys."""
    z = (z + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def dropout_seed(device):
    """A fresh attention-dropout key from the device's default generator, with
    no device read: (its seed, its Philox offset) mixed on the host, and the
    offset advanced, as a device dropout mask draw advances it -- so
    torch.cuda.manual_seed(s) makes the key sequence repeat, the CPU generator
    stays untouched, and nothing blocks on the device (a training step of every
    sharded rank issues no sync for it).  During HIP-graph capture, or on a
    generator without offsets, a host counter per (device, seed) replaces the
    offset (the captured replay reuses the captured key, as any captured
    constant)."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    base = gen.initial_seed()
    if not torch.cuda.is_current_stream_capturing() and hasattr(gen, "get_offset"):
        try:
            off = gen.get_offset()
            gen.set_offset(off + 4)
            return _mix64(_mix64(base) ^ off)
        except RuntimeError:
            pass
    k = (idx, base)
    n = _seed_calls.get(k, 0)
    _seed_calls[k] = n + 1
    return _mix64(_mix64(base ^ 0x5EED) ^ n)


def gat_propagate(graph, edge_index, xw, att, heads, out_channels, negative_slope=0.2, bias=None,
                  return_alpha=False, dropout=0.0, seed=None):
    """Fused GATConv aggregation: returns (out [N, H*C], alpha [E, H] or None).
    dropout > 0: GATConv's training-mode attention dropout on the messages
    (callers check gat_dropout_ok); the keep mask is a hash of (seed, slot, head),
    seed drawn from the device's default generator unless given
    (gat_dropout_keep returns the mask).  alpha is the undropped softmax, as upstream's."""
    _lib.require_device(xw, edge_index, att, bias)
    xw = _f32_2d(xw, "x@W").contiguous()
    H, C = int(heads), int(out_channels)
    if xw.shape[0] == 0:
        # no nodes (hence no edges): an empty output, still connected to xw / bias
        # for autograd -- the kernels are not launched
        out = xw * 0.0 if bias is None else xw * 0.0 + bias
        return out, (xw.new_zeros((edge_index.shape[1], H)) if return_alpha else None)
    drop = None
    if dropout > 0:
        if not (gat_dropout_ok(H, C, dropout) and _gat_train_fwd_ok(graph, xw, H, C)):
            raise ValueError("mi355_mp: fused attention dropout needs 0 < p < 1, H <= 32, C %% 4 == 0 and C/4 a "
                             "power of two <= 64 (got p=%g, H=%d, C=%d)" % (dropout, H, C))
        if seed is None:
            seed = dropout_seed(xw.device)
        drop = (int(seed) & 0xFFFFFFFFFFFFFFFF, float(dropout))
    # autograd.Function.forward always runs with grad disabled: decide here whether
    # a backward can follow (then the forward keeps the pre-bias aggregate)
    train = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (xw, att, bias))
    return _GatPropagate.apply(xw, att, bias, graph, edge_index, H, C, float(negative_slope), bool(return_alpha),
                               train, drop)


class _FeatureTransform(torch.autograd.Function):
    """x @ W with a split-K weight gradient.

    Forward is torch.matmul (hipBLASLt), identical to the reference's
    ``torch.matmul(x, self.weight)`` (GCNConv/GATConv [U5, U6]).  The weight
    gradient x^T g reduces over all N rows into a small [F_in, F_out] matrix:
    as one GEMM it has a handful of output tiles (a few dozen workgroups on
    256 CUs), so it is computed as a batched GEMM over row chunks of
    SPLIT_ROWS (one output tile set per chunk) plus a sum over chunks."""
    SPLIT_ROWS = 8192

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return torch.matmul(x, w)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.matmul(g, w.t())
        if ctx.needs_input_grad[1]:
            n = x.shape[0]
            k = _FeatureTransform.SPLIT_ROWS
            s = n // k
            if s >= 8:
                m = s * k
                xs = x[:m].view(s, k, x.shape[1]).transpose(1, 2)
                gs = g[:m].view(s, k, g.shape[1])
                gw = torch.bmm(xs, gs).sum(0)
                if m < n:
                    gw = gw + torch.matmul(x[m:].t(), g[m:])
            else:
                gw = torch.matmul(x.t(), g)
        return gx, gw


def gemm_rows(x, w, force_generic=False):
    """x @ w (fp32, device) with every output row the k-ordered fmaf chain of
    its own input row (mp_gemm_rows_f32): bitwise independent of how many rows
    x has -- a shard's rows equal the single-GPU rows.  No autograd."""
    nat = _lib.native()
    _lib.require_device(x)
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[0]:
        raise ValueError("gemm_rows: x [M, K] and w [K, N] (got %s and %s)" % (tuple(x.shape), tuple(w.shape)))
    if x.dtype != torch.float32 or w.dtype != torch.float32 or w.device != x.device:
        raise TypeError("gemm_rows: fp32 x and w on one device (got %s / %s on %s / %s)"
                        % (x.dtype, w.dtype, x.device, w.device))
    x = x if (x.stride(1) == 1 and x.stride(0) >= x.shape[1]) else x.contiguous()
    w = w.contiguous()
    M, K = x.shape
    N = w.shape[1]
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    if M and K and N:
        nat.mp_gemm_rows_f32(x.data_ptr(), x.stride(0), M, K, w.data_ptr(), 0, N, out.data_ptr(), N,
                             int(bool(force_generic)), _lib.stream_ptr(x.device))
    elif M and N:
        out.zero_()
    return out


class _FeatureTransformRows(_FeatureTransform):
    """_FeatureTransform with the row-exact forward (gemm_rows); the backward is
    _FeatureTransform's."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return gemm_rows(x, w)


# GATConv / ShardedGATConv: x @ W with the row-exact GEMM, so a sharded layer's
# scores are bitwise the single-GPU layer's
GAT_ROW_EXACT_GEMM = True


def feature_transform(x, w, row_exact=False):
    """``torch.matmul(x, w)`` for a 2-D fp32 device x (split-K weight gradient);
    row_exact: the forward by gemm_rows (each output row a function of its own
    input row, whatever the row count)."""
    if not (torch.is_tensor(x) and x.dim() == 2 and x.is_cuda and x.dtype == torch.float32 and w.dim() == 2):
        return torch.matmul(x, w)
    if not (torch.is_grad_enabled() and (w.requires_grad or x.requires_grad)):
        return gemm_rows(x, w) if row_exact else torch.matmul(x, w)
    if row_exact:
        return _FeatureTransformRows.apply(x, w)
    if not w.requires_grad:
        return torch.matmul(x, w)
    return _FeatureTransform.apply(x, w)


# ---------------------------------------------------------------------------
# SplineConv: fused B-spline aggregation (csrc/mp_spline.hip)
# ---------------------------------------------------------------------------

def _int_list(v):
    if torch.is_tensor(v):
        v = v.reshape(-1).tolist()
    elif isinstance(v, (int, bool)):
        v = [v]
    return [int(a) for a in v]


def _spline_geom(kernel_size, is_open_spline, degree, D, F=1):
    """(ks int32[D], open int32[D], K, S) as the C-ABI takes them (host arrays).
    The limits of the fused path live in one place, mp_spline_ok; a shape it
    refuses raises NotImplementedError with its text, which names the limit."""
    ks = _int_list(kernel_size)
    op = [int(bool(a)) for a in _int_list(is_open_spline)]
    D, degree = int(D), int(degree)
    if len(ks) != D or len(op) != D:
        raise ValueError("mi355_mp: pseudo has %d dimensions, kernel_size %d and is_open_spline %d entries"
                         % (D, len(ks), len(op)))
    ks_a = (_lib.i32 * max(D, 1))(*ks)
    op_a = (_lib.i32 * max(D, 1))(*op)
    nat = _lib.native()
    if not nat.mp_spline_ok(D, degree, ks_a, op_a, max(int(F), 1)):
        raise NotImplementedError("mi355_mp: outside the fused spline path's limits: "
                                  + nat.mp_last_error().decode(errors="replace"))
    K = 1
    for k in ks:
        K *= k
    return ks_a, op_a, K, (degree + 1) ** D


def _spline_pseudo(pseudo):
    if pseudo.dtype != torch.float32:
        raise TypeError("mi355_mp: pseudo must be float32 (got %s)" % pseudo.dtype)
    if pseudo.dim() == 1:
        pseudo = pseudo.unsqueeze(-1)
    if pseudo.dim() != 2:
        raise ValueError("mi355_mp: pseudo must be [edges, dimensions]")
    return pseudo.contiguous()


def spline_basis(pseudo, kernel_size, is_open_spline, degree):
    """(basis [E, S] fp32, weight_index [E, S] int64) of the B-spline basis in
    edge order (mp_spline_basis_f32; torch_spline_conv's SplineBasis)."""
    _lib.require_device(pseudo)
    pseudo = _spline_pseudo(pseudo)
    E, D = pseudo.shape
    ks_a, op_a, _K, S = _spline_geom(kernel_size, is_open_spline, degree, D)
    basis = torch.empty((E, S), dtype=torch.float32, device=pseudo.device)
    wi = torch.empty((E, S), dtype=torch.int64, device=pseudo.device)
    _lib.native().mp_spline_basis_f32(pseudo.data_ptr(), E, D, ks_a, op_a, int(degree), basis.data_ptr(),
                                      _lib.nbytes(basis), wi.data_ptr(), _lib.nbytes(wi),
                                      _lib.stream_ptr(pseudo.device))
    return basis, wi


def spline_bins(csr, pseudo, geom, degree, x, row_scale=None):
    """out[r, k*F + f] = scale[r] * sum over the slots of r and s with wi = k of
    basis * x[col[slot], f] (mp_spline_aggregate_bins_f32); geom from
    _spline_geom.  No autograd."""
    ks_a, op_a, K, _S = geom
    F = x.shape[1]
    out = torch.empty((csr.n_rows, K * F), dtype=torch.float32, device=x.device)
    if csr.n_rows and F:
        _lib.native().mp_spline_aggregate_bins_f32(csr.struct("other"), pseudo.data_ptr(), pseudo.shape[0],
                                                   pseudo.shape[1], ks_a, op_a, int(degree), x.data_ptr(), x.stride(0),
                                                   F, _lib.ptr(row_scale), out.data_ptr(), out.stride(0),
                                                   _lib.stream_ptr(x.device))
    return out


def spline_gather(csr, pseudo, geom, degree, xk, F, row_scale=None, bias=None):
    """out[r, f] = scale[r] * sum over the slots of r and s of
    basis * xk[col[slot], wi*F + f] (+ bias) (mp_spline_aggregate_gather_f32);
    xk [n_cols, K*F].  No autograd."""
    ks_a, op_a, K, _S = geom
    out = torch.empty((csr.n_rows, F), dtype=torch.float32, device=xk.device)
    if csr.n_rows and F:
        _lib.native().mp_spline_aggregate_gather_f32(csr.struct("other"), pseudo.data_ptr(), pseudo.shape[0],
                                                     pseudo.shape[1], ks_a, op_a, int(degree), xk.data_ptr(),
                                                     xk.stride(0), F, _lib.ptr(row_scale), _lib.ptr(bias),
                                                     out.data_ptr(), out.stride(0), _lib.stream_ptr(xk.device))
    return out


# bins kernels above this many kernels hold fewer than 4 waves per 64 KiB workgroup
SPLINE_BINS_FULL_BLOCK = 64


def spline_form(S, f_in, f_out, K=1):
    """The forward's form, as measured (tools/bench_spline.py,
    profiles/spline_conv_bench*.json).  By gathered floats per edge
    the rule would be transform first ('gather': S * Fout floats of x W per
    edge) when S * Fout < Fin, else aggregate first ('bins': Fin floats of x
    per edge); where that rule picks gather (Cora's 1433 -> 16 and 16 -> 7
    with S = 2) gather was never ahead -- the shapes are host-bound and the
    forms differ by less than the spread -- so it is not used.  Gather won at
    one measured shape: the mesh layer 64 -> 64 with K = 125, S = 8, where the
    bins kernel is bound by its LDS (K > 64: at most 2 waves per workgroup)
    and writes K * Fin floats per row.  So: gather when K > 64, Fin >= 64 and
    S * Fout <= 8 * Fin; bins otherwise.  A record of the measured shapes, not
    a model: bins keeps A [N, K * Fin] for the backward, and with a wide Fin a
    caller short of memory should force form='gather'."""
    if K > SPLINE_BINS_FULL_BLOCK and f_in >= 64 and S * f_out <= 8 * f_in:
        return "gather"
    return "bins"


class _SplinePropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, graph, pseudo, geom, degree, reduce, form):
        K, S = geom[2], geom[3]
        f_in, f_out = weight.shape[1], weight.shape[2]
        csr = graph.dst
        scale = None
        if reduce == "mean":
            scale = (1.0 / csr.degree().clamp(min=1).to(torch.float32)).contiguous()
        A = None
        if form == "bins":
            A = spline_bins(csr, pseudo, geom, degree, x, scale)
            wf = weight.reshape(K * f_in, f_out)
            out = torch.matmul(A, wf) if bias is None else torch.addmm(bias, A, wf)
        else:
            xw = torch.matmul(x, weight.permute(1, 0, 2).reshape(f_in, K * f_out))
            out = spline_gather(csr, pseudo, geom, degree, xw, f_out, scale, bias)
        ctx.graph, ctx.geom, ctx.degree = graph, geom, degree
        ctx.has_bias = bias is not None
        # the cached Graph holds its edge_index weakly and builds the transposed CSR
        # on first use, in backward: keep the tensor alive until then
        ctx.save_for_backward(x, weight, pseudo, scale, A if ctx.needs_input_grad[1] else None,
                              graph._edge_index())
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, pseudo, scale, A, _edge_index = ctx.saved_tensors
        graph, geom, degree = ctx.graph, ctx.geom, ctx.degree
        K, S = geom[2], geom[3]
        f_in, f_out = weight.shape[1], weight.shape[2]
        g = g.contiguous()
        gx = gw = gb = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = col_sums(g)
        gs = g if scale is None else g * scale.view(-1, 1)
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        # the transposed pass: rows = source nodes, gathers destination rows of g
        x_by_gather = want_x and S * f_in < f_out
        B = None
        if (want_x and not x_by_gather) or (want_w and A is None):
            B = spline_bins(graph.src, pseudo, geom, degree, gs)            # [n_src, K * Fout]
        if want_x:
            if x_by_gather:
                gk = torch.matmul(gs, weight.reshape(K * f_in, f_out).t())  # [n_dst, K * Fin]
                gx = spline_gather(graph.src, pseudo, geom, degree, gk, f_in)
            else:
                gx = torch.matmul(B, weight.permute(0, 2, 1).reshape(K * f_out, f_in))
        if want_w:
            if A is not None:
                gw = torch.matmul(A.t(), g).view(K, f_in, f_out)            # A carries the row scale
            else:
                gw = torch.matmul(x.t(), B).view(f_in, K, f_out).permute(1, 0, 2).contiguous()
        return gx, gw, gb, None, None, None, None, None, None


def spline_propagate(graph, x, weight, pseudo, kernel_size, is_open_spline, degree, reduce="mean", form=None,
                     bias=None):
    """out[i] = AGGR_{e = (j -> i)} sum_s basis[e, s] * x[j] @ weight[wi[e, s]] (+ bias)

    SplineConv's propagate (torch_spline_conv's SplineBasis + SplineWeighting,
    then scatter_add / scatter_mean) as one segmented pass and one dense GEMM;
    weight [K, Fin, Fout], pseudo [E, D] in [0, 1] in edge order.  reduce 'add'
    or 'mean' (mean divides by max(deg, 1)); form None picks by spline_form,
    'bins' / 'gather' force one.  Deterministic, native forward and backward
    (the same two kernels over the transposed CSR); no gradient for pseudo."""
    if reduce == "max":
        raise NotImplementedError("mi355_mp: spline_propagate has no aggr='max' (add and mean only)")
    if reduce not in ("add", "sum", "mean"):
        raise ValueError("unknown reduce %r" % (reduce,))
    if form not in (None, "bins", "gather"):
        raise ValueError("unknown form %r" % (form,))
    if pseudo.requires_grad:
        raise NotImplementedError("mi355_mp: spline_propagate has no gradient with respect to pseudo")
    _lib.require_device(x, weight, pseudo, bias)
    x = _f32_2d(x, "x")
    if x.stride(0) < max(x.shape[1], 1):
        x = x.contiguous()
    pseudo = _spline_pseudo(pseudo)
    if weight.dtype != torch.float32 or weight.dim() != 3 or weight.shape[1] != x.shape[1]:
        raise ValueError("mi355_mp: weight must be float32 [K, %d, Fout] (got %s %s)"
                         % (x.shape[1], weight.dtype, tuple(weight.shape)))
    geom = _spline_geom(kernel_size, is_open_spline, degree, pseudo.shape[1], max(x.shape[1], weight.shape[2]))
    if weight.shape[0] != geom[2]:
        raise ValueError("mi355_mp: weight holds %d kernels, prod(kernel_size) = %d" % (weight.shape[0], geom[2]))
    if pseudo.shape[0] != graph.dst.n_edges:
        raise ValueError("mi355_mp: pseudo has %d rows, the graph %d edges" % (pseudo.shape[0], graph.dst.n_edges))
    if x.shape[0] != graph.n_src:
        raise ValueError("mi355_mp: x has %d rows, the graph %d source nodes" % (x.shape[0], graph.n_src))
    if form is None:
        form = spline_form(geom[3], weight.shape[1], weight.shape[2], geom[2])
    reduce = "add" if reduce == "sum" else reduce
    return _SplinePropagate.apply(x, weight, bias, graph, pseudo, geom, int(degree), reduce, form)


# ---------------------------------------------------------------------------
# NNConv: factored edge-conditioned aggregation (csrc/mp_nnconv.hip)
# ---------------------------------------------------------------------------

def nnconv_ok(H, c_in, c_out):
    """Whether (H, Cin, Cout) lies inside the fused path's limits (mp_nnconv_ok)."""
    return bool(_lib.native().mp_nnconv_ok(int(H), int(c_in), int(c_out)))


def nnconv_edge_grad_width(H, c_in):
    """The kernel nnconv_edge_grad takes for a shape: 0 = a lane group per (e, h)
    pair (Cin <= 32), else its 32 or 64 lanes per (edge, 32 or 64 values of h)
    (mp_nnconv_edge_grad_width; needs no GPU)."""
    w = int(_lib.native().mp_nnconv_edge_grad_width(int(H), int(c_in)))
    if w < 0:
        raise ValueError("mi355_mp: " + _lib.native().mp_last_error().decode(errors="replace"))
    return w


def _nnconv_rows(t, what):
    t = _f32_2d(t, what)
    return t if t.stride(0) >= max(t.shape[1], 1) else t.contiguous()


def nnconv_bins(csr, h, x, row_scale=None, out=None):
    """Z[r, k*Cin + c] = scale[r] * sum over the slots of r of ht[eid[slot]][k] *
    x[col[slot], c], ht = [h, 1] (mp_nnconv_aggregate_bins_f32); h [E, H] in edge
    order.  out: a [n_rows, >= (H+1)*Cin] tensor to write into.  No autograd."""
    nat = _lib.native()
    h, x = _nnconv_rows(h, "h"), _nnconv_rows(x, "x")
    H, c_in = h.shape[1], x.shape[1]
    if out is None:
        out = torch.empty((csr.n_rows, (H + 1) * c_in), dtype=torch.float32, device=x.device)
    if csr.n_rows:
        _count_call(nat, "mp_nnconv_aggregate_bins_f32", csr.struct("other"), h.data_ptr(), h.shape[0], h.stride(0), H,
                    x.data_ptr(), x.stride(0), c_in, _lib.ptr(row_scale), out.data_ptr(), out.stride(0),
                    _lib.stream_ptr(x.device))
    return out


def nnconv_gather(csr, h, y, F, row_scale=None, bias=None, out=None):
    """out[r, f] = scale[r] * sum over the slots of r and k <= H of ht[eid[slot]][k]
    * y[col[slot], k*F + f] (+ bias) (mp_nnconv_aggregate_gather_f32); y [n_cols,
    (H+1)*F].  No autograd."""
    nat = _lib.native()
    h, y = _nnconv_rows(h, "h"), _nnconv_rows(y, "y")
    H, F = h.shape[1], int(F)
    if out is None:
        out = torch.empty((csr.n_rows, F), dtype=torch.float32, device=y.device)
    if csr.n_rows:
        _count_call(nat, "mp_nnconv_aggregate_gather_f32", csr.struct("other"), h.data_ptr(), h.shape[0], h.stride(0),
                    H, y.data_ptr(), y.stride(0), F, _lib.ptr(row_scale), _lib.ptr(bias), out.data_ptr(),
                    out.stride(0), _lib.stream_ptr(y.device))
    return out


def nnconv_edge_grad(rows, cols, dz, x, H, out=None):
    """dh[e, k] = sum_c dz[rows[e], k*Cin + c] * x[cols[e], c] for k < H
    (mp_nnconv_edge_grad_f32); rows / cols int64 [E], range-checked by the
    caller (a CSR built from them has done it).  out: a contiguous float32 [E, H]
    tensor to write into.  No autograd."""
    nat = _lib.native()
    dz, x = _nnconv_rows(dz, "dz"), _nnconv_rows(x, "x")
    rows, cols = rows.contiguous(), cols.contiguous()
    E, H = rows.numel(), int(H)
    if out is not None and not (out.dtype == torch.float32 and tuple(out.shape) == (E, H) and out.is_contiguous()):
        raise ValueError("mi355_mp: out must be a contiguous float32 [%d, %d] tensor" % (E, H))
    dh = torch.empty((E, H), dtype=torch.float32, device=x.device) if out is None else out
    if E:
        _count_call(nat, "mp_nnconv_edge_grad_f32", rows.data_ptr(), cols.data_ptr(), E, dz.data_ptr(), dz.stride(0),
                    x.data_ptr(), x.stride(0), H, x.shape[1], dh.data_ptr(), dh.stride(0), _lib.nbytes(dh),
                    _lib.stream_ptr(x.device))
    return dh


def nnconv_form(H, c_in, c_out, E, N):
    """The forward's form, by the floats each form moves (a pure function of the
    shape; measured in tools/bench_nnconv.py):
      bins    reads H + Cin floats per edge, writes Z [N, (H+1) Cin] and reads it
              back in the GEMM:            E (H + Cin)            + 2 N (H+1) Cin
      gather  writes Y [N, (H+1) Cout] in the GEMM and gathers H + (H+1) Cout
              floats per edge:             E (H + (H+1) Cout)     +   N (H+1) Cout
    The lower count wins, ties to bins (it keeps Z for the head's gradient, the
    gather form recomputes it in the backward).  Gather is ahead only where Cout
    is far below Cin and the graph is sparse: E (H+1) Cout < N (H+1) (2 Cin -
    Cout) + E Cin.  Every measured shape is ahead of the per-edge recipe in the
    form picked here, so none is sent to the generic path."""
    bins = E * (H + c_in) + 2 * N * (H + 1) * c_in
    gather = E * (H + (H + 1) * c_out) + N * (H + 1) * c_out
    return "bins" if bins <= gather else "gather"


def _nnconv_head_matrix(head_weight, head_bias, c_in, c_out):
    """L [(H+1) Cin, Cout] (H Cin rows without a head bias): L[k*Cin + c, o] =
    head_weight[c*Cout + o, k], rows k = H the head bias -- one permuting copy."""
    H = head_weight.shape[1]
    rows = H + (0 if head_bias is None else 1)
    L = torch.empty((rows * c_in, c_out), dtype=torch.float32, device=head_weight.device)
    L[:H * c_in].view(H, c_in, c_out).copy_(head_weight.reshape(c_in, c_out, H).permute(2, 0, 1))
    if head_bias is not None:
        L[H * c_in:].copy_(head_bias.reshape(c_in, c_out))
    return L


class _NNConvPropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h, head_weight, head_bias, bias, graph, reduce, form):
        H, c_in = h.shape[1], x.shape[1]
        c_out = head_weight.shape[0] // c_in
        csr = graph.dst
        has_hb = head_bias is not None
        used = (H + 1 if has_hb else H)                  # row blocks of L: without a head bias the last is zero
        scale = None
        if reduce == "mean":
            scale = (1.0 / csr.degree().clamp(min=1).to(torch.float32)).contiguous()
        L = _nnconv_head_matrix(head_weight, head_bias, c_in, c_out)
        Z = None
        if form == "bins":
            Z = nnconv_bins(csr, h, x, scale)
            Zu = Z[:, :used * c_in]
            out = torch.mm(Zu, L) if bias is None else torch.addmm(bias, Zu, L)
        else:
            Lp = L.view(used, c_in, c_out).permute(1, 0, 2).reshape(c_in, used * c_out)
            if has_hb:
                Y = torch.mm(x, Lp)
            else:                                        # the kernel reads H + 1 blocks: the last one is zero
                Y = torch.empty((x.shape[0], (H + 1) * c_out), dtype=torch.float32, device=x.device)
                Y[:, :H * c_out] = torch.mm(x, Lp)
                Y[:, H * c_out:].zero_()
            out = nnconv_gather(csr, h, Y, c_out, scale, bias)
        ctx.graph, ctx.has_bias, ctx.has_hb = graph, bias is not None, has_hb
        want_head = ctx.needs_input_grad[2] or (has_hb and ctx.needs_input_grad[3])
        # the cached Graph holds its edge_index weakly and builds the transposed CSR
        # on first use, in backward: keep the tensor alive until then
        ctx.save_for_backward(x, h, L, scale, Z if want_head else None, graph._edge_index())
        return out

    @staticmethod
    def backward(ctx, g):
        x, h, L, scale, Z, edge_index = ctx.saved_tensors
        graph, has_hb = ctx.graph, ctx.has_hb
        H, c_in, c_out = h.shape[1], x.shape[1], L.shape[1]
        used = H + 1 if has_hb else H
        g = g.contiguous()
        gx = gh = gw = ghb = gb = None
        if ctx.has_bias and ctx.needs_input_grad[4]:
            gb = col_sums(g)
        want_x, want_h = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_head = ctx.needs_input_grad[2] or (has_hb and ctx.needs_input_grad[3])
        if want_head:
            if Z is None:                                # the gather form never built it
                Z = nnconv_bins(graph.dst, h, x, scale)
            gL = torch.mm(Z[:, :used * c_in].t(), g)     # Z carries the row scale
            if ctx.needs_input_grad[2]:
                gw = gL[:H * c_in].view(H, c_in, c_out).permute(1, 2, 0).reshape(c_in * c_out, H)
            if has_hb and ctx.needs_input_grad[3]:
                ghb = gL[H * c_in:].reshape(c_in * c_out)
        if want_x or want_h:
            gs = g if scale is None else g * scale.view(-1, 1)
            if has_hb:
                dZ = torch.mm(gs, L.t())
            else:
                dZ = torch.empty((g.shape[0], (H + 1) * c_in), dtype=torch.float32, device=g.device)
                dZ[:, :H * c_in] = torch.mm(gs, L.t())
                dZ[:, H * c_in:].zero_()
            if want_x:
                # the transposed pass: rows = source nodes, gathers destination rows of dZ
                gx = nnconv_gather(graph.src, h, dZ, c_in)
            if want_h:
                gh = nnconv_edge_grad(edge_index[graph.i], edge_index[graph.j], dZ, x, H)
        return gx, gh, gw, ghb, gb, None, None, None


def nnconv_propagate(graph, x, h, head_weight, head_bias, reduce, form=None, bias=None):
    """out[i] = AGGR_{e = (j -> i)} x[j] @ reshape(head_weight @ h[e] + head_bias, [Cin, Cout]) (+ bias)

    NNConv's propagate for an edge network ending in a Linear (the head), with
    no per-edge weight matrix: one segmented pass and one node-level GEMM.  h
    [E, H] is the head's input in edge order, head_weight [Cin*Cout, H],
    head_bias [Cin*Cout] or None (then the bias row block of L does not exist).
    reduce 'add' or 'mean' (mean divides by max(deg, 1)); form None picks by
    nnconv_form, 'bins' / 'gather' force one.  Deterministic, native forward and
    backward: d x by the gather kernel over the transposed CSR, d h by the
    edge-grad kernel (skipped when h needs no gradient), d head by Z^T g with Z
    saved by the bins form and recomputed after the gather form."""
    if reduce == "max":
        raise NotImplementedError("mi355_mp: nnconv_propagate has no aggr='max' (add and mean only)")
    if reduce not in ("add", "sum", "mean"):
        raise ValueError("unknown reduce %r" % (reduce,))
    if form not in (None, "bins", "gather"):
        raise ValueError("unknown form %r" % (form,))
    _lib.require_device(x, h, head_weight, head_bias, bias)
    # x also feeds a GEMM (x L' of the gather form), whose rounding follows the operand layout: one layout
    x, h = _f32_2d(x, "x").contiguous(), _nnconv_rows(h, "h")
    H, c_in = h.shape[1], x.shape[1]
    if head_weight.dtype != torch.float32 or head_weight.dim() != 2 or head_weight.shape[1] != H \
            or c_in == 0 or head_weight.shape[0] % max(c_in, 1):
        raise ValueError("mi355_mp: head_weight must be float32 [%d * Cout, %d] (got %s %s)"
                         % (c_in, H, head_weight.dtype, tuple(head_weight.shape)))
    c_out = head_weight.shape[0] // c_in
    if head_bias is not None and tuple(head_bias.shape) != (c_in * c_out,):
        raise ValueError("mi355_mp: head_bias must be [%d] (got %s)" % (c_in * c_out, tuple(head_bias.shape)))
    if not nnconv_ok(H, c_in, c_out):
        raise NotImplementedError("mi355_mp: outside the fused NNConv path's limits: "
                                  + _lib.native().mp_last_error().decode(errors="replace"))
    if h.shape[0] != graph.dst.n_edges:
        raise ValueError("mi355_mp: h has %d rows, the graph %d edges" % (h.shape[0], graph.dst.n_edges))
    if x.shape[0] != graph.n_src:
        raise ValueError("mi355_mp: x has %d rows, the graph %d source nodes" % (x.shape[0], graph.n_src))
    if form is None:
        form = nnconv_form(H, c_in, c_out, h.shape[0], x.shape[0])
    reduce = "add" if reduce == "sum" else reduce
    return _NNConvPropagate.apply(x, h, head_weight, head_bias, bias, graph, reduce, form)


# ---------------------------------------------------------------------------
# GMMConv: Gaussian mixture weights fused into the aggregation (csrc/mp_gmm.hip)
# ---------------------------------------------------------------------------

def gmm_ok(K, D, c_in, c_out):
    """Whether (K, D, Cin, Cout) lies inside the fused path's limits (mp_gmm_ok; needs no GPU)."""
    return bool(_lib.native().mp_gmm_ok(int(K), int(D), int(c_in), int(c_out)))


def gmm_grad_chunk(n_edges, K, D):
    """Edges per stage-1 workgroup of gmm_param_grad: a pure function of the shape
    (mp_gmm_grad_chunk; needs no GPU)."""
    c = int(_lib.native().mp_gmm_grad_chunk(int(n_edges), int(K), int(D)))
    if c < 0:
        raise ValueError("mi355_mp: " + _lib.native().mp_last_error().decode(errors="replace"))
    return c


def _gmm_table(mu, sigma):
    if mu.dtype != torch.float32 or sigma.dtype != torch.float32 or mu.dim() != 2 or mu.shape != sigma.shape:
        raise ValueError("mi355_mp: mu and sigma must be float32 [K, D] (got %s %s, %s %s)"
                         % (mu.dtype, tuple(mu.shape), sigma.dtype, tuple(sigma.shape)))
    return mu.detach().contiguous(), sigma.detach().contiguous()


def gmm_bins(csr, pseudo, mu, sigma, x, row_scale=None, out=None):
    """Z[r, k*Cin + c] = scale[r] * sum over the slots of r of w_k(pseudo[eid[slot]]) *
    x[col[slot], c] (mp_gmm_aggregate_bins_f32); pseudo [E, D] in edge order, mu /
    sigma [K, D].  out: a [n_rows, >= K*Cin] tensor to write into.  No autograd."""
    nat = _lib.native()
    pseudo, x = _nnconv_rows(pseudo, "pseudo"), _nnconv_rows(x, "x")
    mu, sigma = _gmm_table(mu, sigma)
    (K, D), c_in = mu.shape, x.shape[1]
    if pseudo.shape[1] != D:
        raise ValueError("mi355_mp: pseudo has %d columns, mu %d" % (pseudo.shape[1], D))
    if out is None:
        out = torch.empty((csr.n_rows, K * c_in), dtype=torch.float32, device=x.device)
    if csr.n_rows:
        _count_call(nat, "mp_gmm_aggregate_bins_f32", csr.struct("other"), pseudo.data_ptr(), pseudo.shape[0],
                    pseudo.stride(0), D, mu.data_ptr(), sigma.data_ptr(), K, x.data_ptr(), x.stride(0), c_in,
                    _lib.ptr(row_scale), out.data_ptr(), out.stride(0), _lib.stream_ptr(x.device))
    return out


def gmm_gather(csr, pseudo, mu, sigma, y, F, row_scale=None, bias=None, out=None):
    """out[r, f] = scale[r] * sum over the slots of r and k < K (k ascending) of
    w_k(pseudo[eid[slot]]) * y[col[slot], k*F + f] (+ bias) (mp_gmm_aggregate_gather_f32);
    y [n_cols, K*F].  No autograd."""
    nat = _lib.native()
    pseudo, y = _nnconv_rows(pseudo, "pseudo"), _nnconv_rows(y, "y")
    mu, sigma = _gmm_table(mu, sigma)
    (K, D), F = mu.shape, int(F)
    if pseudo.shape[1] != D:
        raise ValueError("mi355_mp: pseudo has %d columns, mu %d" % (pseudo.shape[1], D))
    if out is None:
        out = torch.empty((csr.n_rows, F), dtype=torch.float32, device=y.device)
    if csr.n_rows:
        _count_call(nat, "mp_gmm_aggregate_gather_f32", csr.struct("other"), pseudo.data_ptr(), pseudo.shape[0],
                    pseudo.stride(0), D, mu.data_ptr(), sigma.data_ptr(), K, y.data_ptr(), y.stride(0), F,
                    _lib.ptr(row_scale), _lib.ptr(bias), out.data_ptr(), out.stride(0), _lib.stream_ptr(y.device))
    return out


def gmm_param_grad(rows, cols, pseudo, mu, sigma, dz, x, want_pseudo=False, dmu=None, dsigma=None, dpseudo=None):
    """(dmu, dsigma, dpseudo or None) of mp_gmm_param_grad_f32: with dw[e, k] = sum_c
    dz[rows[e], k*Cin + c] * x[cols[e], c] and t = dw * w_k(pseudo[e]), dmu[k, d] =
    sum_e t (p_d - mu_kd) iv_kd, dsigma[k, d] = sum_e t ((p_d - mu_kd)^2 iv_kd)
    (sigma_kd iv_kd), dpseudo[e, d] = -sum_k t (p_d - mu_kd) iv_kd.  Chunk partials
    in a fixed order, then the chunks in order: bitwise reproducible.  rows / cols
    int64 [E], range-checked by the caller (a CSR built from them has done it);
    dpseudo is computed only with want_pseudo (or a dpseudo= tensor to write
    into).  No autograd."""
    nat = _lib.native()
    pseudo, dz, x = _nnconv_rows(pseudo, "pseudo"), _nnconv_rows(dz, "dz"), _nnconv_rows(x, "x")
    mu, sigma = _gmm_table(mu, sigma)
    rows, cols = rows.contiguous(), cols.contiguous()
    (K, D), E = mu.shape, rows.numel()
    if cols.numel() != E or pseudo.shape[0] != E or pseudo.shape[1] != D:
        raise ValueError("mi355_mp: rows / cols / pseudo must hold %d edges and pseudo %d columns (got %d, %s)"
                         % (E, D, cols.numel(), tuple(pseudo.shape)))
    for t, what in ((dmu, "dmu"), (dsigma, "dsigma")):
        if t is not None and not (t.dtype == torch.float32 and tuple(t.shape) == (K, D) and t.is_contiguous()):
            raise ValueError("mi355_mp: %s must be a contiguous float32 [%d, %d] tensor" % (what, K, D))
    dmu = torch.empty((K, D), dtype=torch.float32, device=x.device) if dmu is None else dmu
    dsigma = torch.empty((K, D), dtype=torch.float32, device=x.device) if dsigma is None else dsigma
    if dpseudo is None and want_pseudo:
        dpseudo = torch.empty((E, D), dtype=torch.float32, device=x.device)
    if dpseudo is not None and not (dpseudo.dtype == torch.float32 and dpseudo.dim() == 2
                                    and tuple(dpseudo.shape) == (E, D) and dpseudo.stride(1) in (0, 1)
                                    and dpseudo.stride(0) >= D):
        raise ValueError("mi355_mp: dpseudo must be a float32 [%d, %d] tensor with unit column stride" % (E, D))
    ws_bytes = nat.mp_gmm_param_grad_workspace(E, K, D)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    _count_call(nat, "mp_gmm_param_grad_f32", rows.data_ptr(), cols.data_ptr(), E, pseudo.data_ptr(), pseudo.stride(0),
                D, mu.data_ptr(), sigma.data_ptr(), K, dz.data_ptr(), dz.stride(0), x.data_ptr(), x.stride(0),
                x.shape[1], dmu.data_ptr(), dsigma.data_ptr(), _lib.ptr(dpseudo),
                0 if dpseudo is None else dpseudo.stride(0), ws.data_ptr(), ws_bytes, _lib.stream_ptr(x.device))
    return dmu, dsigma, dpseudo


def gmm_form(K, D, c_in, c_out, E, N):
    """The forward's form, by the floats each form moves (a pure function of the shape):
      bins    reads D + Cin floats per edge, writes Z [N, K Cin] and reads it back
              in the GEMM:                 E (D + Cin)        + 2 N K Cin
      gather  writes Y [N, K Cout] in the GEMM and gathers D + K Cout floats per
              edge:                        E (D + K Cout)     +   N K Cout
    The lower count wins, ties to bins (it keeps Z for g's gradient, the gather
    form recomputes it in the backward)."""
    bins = E * (D + c_in) + 2 * N * K * c_in
    gather = E * (D + K * c_out) + N * K * c_out
    return "bins" if bins <= gather else "gather"


def _gmm_mix_matrix(g, K, c_in, c_out):
    """G' [K Cin, Cout]: G'[k*Cin + c, m] = g[c, k*Cout + m] -- one permuting copy."""
    return g.detach().view(c_in, K, c_out).permute(1, 0, 2).reshape(K * c_in, c_out)


class _GMMPropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pseudo, mu, sigma, g, bias, graph, reduce, form):
        (K, D), c_in = mu.shape, x.shape[1]
        c_out = g.shape[1] // K
        csr = graph.dst
        scale = None
        if reduce == "mean":
            scale = (1.0 / csr.degree().clamp(min=1).to(torch.float32)).contiguous()
        Z = None
        if form == "bins":
            Gp = _gmm_mix_matrix(g, K, c_in, c_out)
            Z = gmm_bins(csr, pseudo, mu, sigma, x, scale)
            out = torch.mm(Z, Gp) if bias is None else torch.addmm(bias, Z, Gp)
        else:
            Y = torch.mm(x, g)                           # [N, K, Cout]: g's own column order
            out = gmm_gather(csr, pseudo, mu, sigma, Y, c_out, scale, bias)
        ctx.graph, ctx.has_bias = graph, bias is not None
        # the cached Graph holds its edge_index weakly and builds the transposed CSR
        # on first use, in backward: keep the tensor alive until then
        ctx.save_for_backward(x, pseudo, mu, sigma, g, scale, Z if ctx.needs_input_grad[4] else None,
                              graph._edge_index())
        return out

    @staticmethod
    def backward(ctx, go):
        x, pseudo, mu, sigma, g, scale, Z, edge_index = ctx.saved_tensors
        graph = ctx.graph
        (K, D), c_in = mu.shape, x.shape[1]
        c_out = g.shape[1] // K
        go = go.contiguous()
        gx = gp = gmu = gsigma = gg = gb = None
        if ctx.has_bias and ctx.needs_input_grad[5]:
            gb = col_sums(go)
        if ctx.needs_input_grad[4]:
            if Z is None:                                # the gather form never built it
                Z = gmm_bins(graph.dst, pseudo, mu, sigma, x, scale)
            gGp = torch.mm(Z.t(), go)                    # Z carries the row scale
            gg = gGp.view(K, c_in, c_out).permute(1, 0, 2).reshape(c_in, K * c_out)
        want_x = ctx.needs_input_grad[0]
        want_p, want_mu, want_sigma = ctx.needs_input_grad[1:4]
        if want_x or want_p or want_mu or want_sigma:
            gs = go if scale is None else go * scale.view(-1, 1)
            dZ = torch.mm(gs, _gmm_mix_matrix(g, K, c_in, c_out).t())
            if want_x:
                # the transposed pass: rows = source nodes, gathers destination rows of dZ
                gx = gmm_gather(graph.src, pseudo, mu, sigma, dZ, c_in)
            if want_p or want_mu or want_sigma:
                gmu, gsigma, gp = gmm_param_grad(edge_index[graph.i], edge_index[graph.j], pseudo, mu, sigma, dZ, x,
                                                 want_pseudo=want_p)
                gmu = gmu if want_mu else None
                gsigma = gsigma if want_sigma else None
        return gx, gp, gmu, gsigma, gg, gb, None, None, None


def gmm_propagate(graph, x, pseudo, mu, sigma, g, reduce, form=None, bias=None):
    """out[i] = AGGR_{e = (j -> i)} sum_k w_k(pseudo[e]) * (x[j] @ g)[k*M : (k+1)*M] (+ bias),
    w_k(p) = exp(sum_d -0.5 (p_d - mu_kd)^2 / (1e-15 + sigma_kd^2))

    GMMConv's propagate with shared Gaussians: the weights are evaluated inside
    one segmented pass, plus one node-level GEMM; no [E, K, M] or [E, K] array.
    pseudo [E, D] in edge order, mu / sigma [K, D], g [Cin, K*M].  reduce 'add'
    or 'mean' (mean divides by max(deg, 1)); form None picks by gmm_form, 'bins'
    / 'gather' force one.  Deterministic, native forward and backward: d x by the
    gather kernel over the transposed CSR, d g by Z^T g_out with Z saved by the
    bins form and recomputed after the gather form, d mu / d sigma / d pseudo by
    gmm_param_grad (skipped when none of the three needs a gradient)."""
    if reduce == "max":
        raise NotImplementedError("mi355_mp: gmm_propagate has no aggr='max' (add and mean only)")
    if reduce not in ("add", "sum", "mean"):
        raise ValueError("unknown reduce %r" % (reduce,))
    if form not in (None, "bins", "gather"):
        raise ValueError("unknown form %r" % (form,))
    _lib.require_device(x, pseudo, mu, sigma, g, bias)
    # x also feeds a GEMM (x g of the gather form), whose rounding follows the operand layout: one layout
    x, pseudo = _f32_2d(x, "x").contiguous(), _nnconv_rows(pseudo, "pseudo")
    if mu.dtype != torch.float32 or sigma.dtype != torch.float32 or mu.dim() != 2 or mu.shape != sigma.shape:
        raise ValueError("mi355_mp: mu and sigma must be float32 [K, D] (got %s %s, %s %s)"
                         % (mu.dtype, tuple(mu.shape), sigma.dtype, tuple(sigma.shape)))
    (K, D), c_in = mu.shape, x.shape[1]
    if pseudo.shape[1] != D:
        raise ValueError("mi355_mp: pseudo has %d columns, mu %d" % (pseudo.shape[1], D))
    if g.dtype != torch.float32 or g.dim() != 2 or g.shape[0] != c_in or K == 0 or g.shape[1] % max(K, 1):
        raise ValueError("mi355_mp: g must be float32 [%d, %d * Cout] (got %s %s)"
                         % (c_in, K, g.dtype, tuple(g.shape)))
    c_out = g.shape[1] // K
    if bias is not None and tuple(bias.shape) != (c_out,):
        raise ValueError("mi355_mp: bias must be [%d] (got %s)" % (c_out, tuple(bias.shape)))
    if not gmm_ok(K, D, c_in, c_out):
        raise NotImplementedError("mi355_mp: outside the fused GMMConv path's limits: "
                                  + _lib.native().mp_last_error().decode(errors="replace"))
    if pseudo.shape[0] != graph.dst.n_edges:
        raise ValueError("mi355_mp: pseudo has %d rows, the graph %d edges" % (pseudo.shape[0], graph.dst.n_edges))
    if x.shape[0] != graph.n_src:
        raise ValueError("mi355_mp: x has %d rows, the graph %d source nodes" % (x.shape[0], graph.n_src))
    if form is None:
        form = gmm_form(K, D, c_in, c_out, pseudo.shape[0], x.shape[0])
    reduce = "add" if reduce == "sum" else reduce
    return _GMMPropagate.apply(x, pseudo, mu, sigma, g.contiguous(), bias, graph, reduce, form)


# ---------------------------------------------------------------------------
# RGCNConv: relational aggregation over a basis decomposition (csrc/mp_rgcn.hip)
# ---------------------------------------------------------------------------

def rgcn_ok(R, B, c_in, c_out):
    """Whether (R, B, Cin, Cout) lies inside the fused path's limits (mp_rgcn_ok)."""
    return bool(_lib.native().mp_rgcn_ok(int(R), int(B), int(c_in), int(c_out)))


def rgcn_att_chunk():
    """Edges of one relation per stage-1 workgroup of rgcn_att_grad (mp_rgcn_att_chunk; needs no GPU)."""
    return int(_lib.native().mp_rgcn_att_chunk())


class RelationPlan(object):
    """The edges grouped by relation: perm (device int64 [E], the edge ids stably
    sorted by type) and relptr (device int64 [R + 1]; relation r owns positions
    [relptr[r], relptr[r + 1]) of perm).  Every type lies in [0, R)."""
    __slots__ = ("perm", "relptr", "n_relations", "n_edges")

    def __init__(self, perm, relptr, n_relations, n_edges):
        self.perm, self.relptr, self.n_relations, self.n_edges = perm, relptr, n_relations, n_edges


_rgcn_plan_cache = _Cache()


def rgcn_relation_plan(edge_type, R):
    """RelationPlan of edge_type (int64 [E] on the device) for R relations: one
    stable device sort, whose two ends are the range check -- a type outside
    [0, R) raises IndexError here, before any kernel reads att with it.  Cached
    on the edge_type tensor (identity + version counter, as the CSR and batch
    layout caches): one sort and one host read the first time a tensor is seen."""
    _lib.require_device(edge_type)
    if edge_type.dtype != torch.int64 or edge_type.dim() != 1:
        raise TypeError("mi355_mp: edge_type must be int64 [E] (got %s %s)" % (edge_type.dtype, tuple(edge_type.shape)))
    R = int(R)

    def build():
        E, dev = edge_type.numel(), edge_type.device
        if E == 0:
            return RelationPlan(torch.empty(0, dtype=torch.int64, device=dev),
                                torch.zeros(R + 1, dtype=torch.int64, device=dev), R, 0)
        types, perm = torch.sort(edge_type, stable=True)
        lo, hi = torch.stack([types[0], types[-1]]).tolist()
        if lo < 0 or hi >= R:
            raise IndexError("mi355_mp: edge_type holds values in [%d, %d], the layer has relations 0..%d"
                             % (lo, hi, R - 1))
        relptr = torch.searchsorted(types, torch.arange(R + 1, dtype=torch.int64, device=dev))
        return RelationPlan(perm.contiguous(), relptr.contiguous(), R, E)

    return _rgcn_plan_cache.get(edge_type, ("rgcn_plan", edge_type.data_ptr(), R), build)


def _extent_bytes(t):
    """Bytes from a strided tensor's first element to one past its last (its numel
    times the element size when it is contiguous; 0 for an empty one)."""
    if t.numel() == 0:
        return 0
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


def _rgcn_coef(csr, edge_type, edge_norm, att):
    """The arguments every aggregate call reads a slot's coefficients through."""
    att = _nnconv_rows(att, "att")
    edge_type = edge_type.contiguous()
    if edge_norm is not None:
        if edge_norm.dtype != torch.float32 or edge_norm.dim() != 1 or edge_norm.numel() != edge_type.numel():
            raise ValueError("mi355_mp: edge_norm must be float32 [%d] (got %s %s)"
                             % (edge_type.numel(), edge_norm.dtype, tuple(edge_norm.shape)))
        edge_norm = edge_norm.detach().contiguous()
    keep = (att, edge_type, edge_norm)
    return keep, (csr.struct("other"), edge_type.data_ptr(), _lib.ptr(edge_norm), edge_type.numel(), att.data_ptr(),
                  att.stride(0), _extent_bytes(att), att.shape[0], att.shape[1])


def _rgcn_blocks(t, what):
    """A [B, n, C] operand addressed in place: (tensor, ld_node, ld_block)."""
    if t.dtype != torch.float32 or t.dim() != 3:
        raise TypeError("mi355_mp: %s must be float32 [B, n, C] (got %s %s)" % (what, t.dtype, tuple(t.shape)))
    if t.stride(2) != 1 or t.stride(1) < t.shape[2] or t.stride(0) < t.shape[1] * t.stride(1):
        t = t.contiguous()
    return t, t.stride(1), t.stride(0)


def rgcn_bins(csr, edge_type, edge_norm, att, x, out=None):
    """out[r, b, c] = sum over the slots of r of (norm[eid] * att[type[eid], b]) *
    x[col[slot], c] (mp_rgcn_aggregate_bins_f32); edge_type int64 [E] and edge_norm
    (fp32 [E] or None = 1) in edge order, att [R, B], types range-checked by the
    caller (rgcn_relation_plan).  out: None or a 2-D tensor [n_rows, >= B*C] (Z:
    entry (b, c) of a row at b*C + c), or a 3-D tensor [B, n_rows, C] written in
    place through its strides (d basis of the featureless layer).  No autograd."""
    nat = _lib.native()
    x = _nnconv_rows(x, "x")
    keep, coef = _rgcn_coef(csr, edge_type, edge_norm, att)
    B, C = keep[0].shape[1], x.shape[1]
    if out is None:
        out = torch.empty((csr.n_rows, B * C), dtype=torch.float32, device=x.device)
    if out.dim() == 3:
        if tuple(out.shape) != (B, csr.n_rows, C) or out.stride(2) != 1:
            raise ValueError("mi355_mp: a 3-D out must be [%d, %d, %d] with unit stride in c" % (B, csr.n_rows, C))
        ld_node, ld_block = out.stride(1), out.stride(0)
    else:
        ld_node, ld_block = out.stride(0), C
    if csr.n_rows:
        _count_call(nat, "mp_rgcn_aggregate_bins_f32", *coef, x.data_ptr(), x.stride(0), C, out.data_ptr(), ld_node,
                    ld_block, _extent_bytes(out), _lib.stream_ptr(x.device))
    return out


def rgcn_gather(csr, edge_type, edge_norm, att, y, F=None, bias=None, out=None):
    """out[r, f] = sum over the slots of r and b < B of (norm[eid] * att[type[eid], b])
    * y[col[slot], b, f] (+ bias) (mp_rgcn_aggregate_gather_f32).  y: a 2-D tensor
    [n_cols, >= B*F] (entry (b, f) of a row at b*F + f; F required), or a 3-D
    tensor [B, n_cols, F] read in place through its strides (basis itself, for
    the featureless layer).  No autograd."""
    nat = _lib.native()
    keep, coef = _rgcn_coef(csr, edge_type, edge_norm, att)
    if y.dim() == 3:
        y, ld_node, ld_block = _rgcn_blocks(y, "y")
        F = y.shape[2]
    else:
        y, F = _nnconv_rows(y, "y"), int(F)
        ld_node, ld_block = y.stride(0), F
    if out is None:
        out = torch.empty((csr.n_rows, F), dtype=torch.float32, device=y.device)
    if csr.n_rows:
        _count_call(nat, "mp_rgcn_aggregate_gather_f32", *coef, y.data_ptr(), ld_node, ld_block, _extent_bytes(y), F,
                    _lib.ptr(bias), out.data_ptr(), out.stride(0), _lib.stream_ptr(y.device))
    return out


def rgcn_att_grad(plan, rows, cols, edge_norm, P, Q, B, out=None):
    """datt[r, b] = sum over the edges e of relation r of norm[e] * sum_c P[rows[e], b,
    c] * Q[cols[e], c] (mp_rgcn_att_grad_f32): chunk partials in a fixed order,
    then the relation's chunks in chunk order; zeros for a relation without
    edges.  P: a 2-D tensor [n, >= B*C] or a 3-D one [B, n, C] read in place; Q
    [m, C]; rows / cols int64 [E], range-checked by the caller (a CSR built from
    them has done it).  out: a contiguous float32 [R, B] tensor to write into.
    No autograd."""
    nat = _lib.native()
    Q = _nnconv_rows(Q, "Q")
    C, B = Q.shape[1], int(B)
    if P.dim() == 3:
        P, ldp_node, ldp_block = _rgcn_blocks(P, "P")
    else:
        P = _nnconv_rows(P, "P")
        ldp_node, ldp_block = P.stride(0), C
    rows, cols = rows.contiguous(), cols.contiguous()
    R, E = plan.n_relations, plan.n_edges
    if rows.numel() != E or cols.numel() != E:
        raise ValueError("mi355_mp: the relation plan holds %d edges, rows / cols %d / %d" % (E, rows.numel(), cols.numel()))
    if edge_norm is not None:
        if edge_norm.dtype != torch.float32 or edge_norm.numel() != E:
            raise ValueError("mi355_mp: edge_norm must be float32 [%d] (got %s %s)"
                             % (E, edge_norm.dtype, tuple(edge_norm.shape)))
        edge_norm = edge_norm.detach().contiguous()
    if out is not None and not (out.dtype == torch.float32 and tuple(out.shape) == (R, B) and out.is_contiguous()):
        raise ValueError("mi355_mp: out must be a contiguous float32 [%d, %d] tensor" % (R, B))
    datt = torch.empty((R, B), dtype=torch.float32, device=Q.device) if out is None else out
    ws_bytes = nat.mp_rgcn_att_grad_workspace(E, R, B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=Q.device)
    _count_call(nat, "mp_rgcn_att_grad_f32", plan.perm.data_ptr(), plan.relptr.data_ptr(), rows.data_ptr(),
                cols.data_ptr(), E, _lib.ptr(edge_norm), P.data_ptr(), ldp_node, ldp_block, Q.data_ptr(), Q.stride(0),
                R, B, C, datt.data_ptr(), datt.stride(0), _lib.nbytes(datt), ws.data_ptr(), ws_bytes,
                _lib.stream_ptr(Q.device))
    return datt


def rgcn_form(B, c_in, c_out, E, N):
    """The featured forward's form, by the floats each form moves (a pure
    function of the shape; measured in tools/bench_rgcn.py):
      bins    reads B + Cin floats per edge, writes Z [N, B Cin] and reads it
              back in the GEMM:            E (B + Cin)          + 2 N B Cin
      gather  writes Y [N, B Cout] in the GEMM and gathers B + B Cout floats
              per edge:                    E (B + B Cout)       +   N B Cout
    The lower count wins, ties to bins (it keeps Z for d basis, the gather form
    recomputes it in the backward).  The featureless layer has one form."""
    bins = E * (B + c_in) + 2 * N * B * c_in
    gather = E * (B + B * c_out) + N * B * c_out
    return "bins" if bins <= gather else "gather"


class _RGCNPropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, basis, att, bias, graph, edge_type, edge_norm, plan, form):
        B, c_in, c_out = basis.shape
        csr = graph.dst
        Z = None
        if x is None:                                    # x = identity: row j of every basis[b], in place
            out = rgcn_gather(csr, edge_type, edge_norm, att, basis, bias=bias)
        elif form == "bins":
            Z = rgcn_bins(csr, edge_type, edge_norm, att, x)
            V = basis.view(B * c_in, c_out)
            out = torch.mm(Z, V) if bias is None else torch.addmm(bias, Z, V)
        else:
            Y = torch.mm(x, basis.permute(1, 0, 2).reshape(c_in, B * c_out))
            out = rgcn_gather(csr, edge_type, edge_norm, att, Y, c_out, bias=bias)
        ctx.graph, ctx.plan, ctx.has_bias, ctx.featureless = graph, plan, bias is not None, x is None
        # the cached Graph holds its edge_index weakly and builds the transposed CSR
        # on first use, in backward: keep the tensor alive until then
        ctx.save_for_backward(x, basis, att, edge_type, edge_norm, Z if ctx.needs_input_grad[1] else None,
                              graph._edge_index())
        return out

    @staticmethod
    def backward(ctx, g):
        x, basis, att, edge_type, edge_norm, Z, edge_index = ctx.saved_tensors
        graph, plan = ctx.graph, ctx.plan
        B, c_in, c_out = basis.shape
        g = g.contiguous()
        gx = gbasis = gatt = gb = None
        if ctx.has_bias and ctx.needs_input_grad[3]:
            gb = col_sums(g)
        want_x, want_basis, want_att = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dst, src = edge_index[graph.i], edge_index[graph.j]
        if ctx.featureless:
            if want_basis:
                # the transposed pass: rows = source nodes j, gathers destination rows of g, written into
                # d basis [B, N, Cout] through the block stride
                gbasis = torch.empty_like(basis, memory_format=torch.contiguous_format)
                rgcn_bins(graph.src, edge_type, edge_norm, att, g, out=gbasis)
            if want_att:
                gatt = rgcn_att_grad(plan, src, dst, edge_norm, basis, g, B)
            return None, gbasis, gatt, gb, None, None, None, None, None
        if want_basis:
            if Z is None:                                # the gather form never built it
                Z = rgcn_bins(graph.dst, edge_type, edge_norm, att, x)
            gbasis = torch.mm(Z.t(), g).view(B, c_in, c_out)
        if want_x or want_att:
            dZ = torch.mm(g, basis.view(B * c_in, c_out).t())
            if want_x:
                gx = rgcn_gather(graph.src, edge_type, edge_norm, att, dZ, c_in)
            if want_att:
                gatt = rgcn_att_grad(plan, dst, src, edge_norm, dZ, x, B)
        return gx, gbasis, gatt, gb, None, None, None, None, None


def rgcn_propagate(graph, x, edge_type, edge_norm, att, basis, root=None, bias=None, form=None):
    """out[i] = sum_{e = (j -> i)} edge_norm[e] * x[j] @ (sum_b att[edge_type[e], b] basis[b]) (+ x[i] @ root) (+ bias)

    RGCNConv's propagate with no per-edge weight matrix: one segmented pass and
    one node-level GEMM.  basis [B, Cin, Cout], att [R, B], edge_type int64 [E]
    (range-checked once per tensor: IndexError), edge_norm fp32 [E] without a
    gradient, or None.  x [N, Cin], or None for the featureless layer (x = the
    identity, N = Cin): then basis is gathered in place, no [R*N, Cout] table is
    built, and root [N, Cout] is added as it is.  form None picks by rgcn_form,
    'bins' / 'gather' force one (featured only).  Deterministic, native forward
    and backward: d x by the gather kernel over the transposed CSR, d basis = Z^T g
    (Z saved by the bins form, recomputed after the gather form; featureless: the
    bins kernel over the transposed CSR, in place), d att by rgcn_att_grad; a
    launch is skipped when nothing needs its gradient."""
    if form not in (None, "bins", "gather"):
        raise ValueError("unknown form %r" % (form,))
    _lib.require_device(x, edge_type, edge_norm, att, basis, root, bias)
    if basis.dtype != torch.float32 or basis.dim() != 3:
        raise ValueError("mi355_mp: basis must be float32 [B, Cin, Cout] (got %s %s)" % (basis.dtype, tuple(basis.shape)))
    B, c_in, c_out = basis.shape
    if att.dtype != torch.float32 or att.dim() != 2 or att.shape[1] != B:
        raise ValueError("mi355_mp: att must be float32 [R, %d] (got %s %s)" % (B, att.dtype, tuple(att.shape)))
    R = att.shape[0]
    if edge_norm is not None and edge_norm.requires_grad:
        raise NotImplementedError("mi355_mp: rgcn_propagate has no gradient with respect to edge_norm")
    if x is not None:
        # one layout for the kernels and the GEMMs (x root, x L'): the GEMM library picks its kernel by the
        # operand layout, so a strided or transposed view of x would round differently from its contiguous copy
        x = _f32_2d(x, "x").contiguous()
        if x.shape[1] != c_in:
            raise ValueError("mi355_mp: x has %d columns, basis %d input channels" % (x.shape[1], c_in))
    elif form is not None:
        raise ValueError("mi355_mp: the featureless layer (x = None) has one form (got form=%r)" % (form,))
    n = c_in if x is None else x.shape[0]
    # the featureless kernels see rows of B * Cout floats only: Cin = N is a node count there
    if not rgcn_ok(R, B, c_out if x is None else c_in, c_out):
        raise NotImplementedError("mi355_mp: outside the fused RGCN path's limits: "
                                  + _lib.native().mp_last_error().decode(errors="replace"))
    if edge_type.numel() != graph.dst.n_edges:
        raise ValueError("mi355_mp: edge_type has %d entries, the graph %d edges" % (edge_type.numel(), graph.dst.n_edges))
    if n != graph.n_src or n != graph.n_dst:
        raise ValueError("mi355_mp: %d nodes, the graph %d sources and %d destinations" % (n, graph.n_src, graph.n_dst))
    plan = rgcn_relation_plan(edge_type, R)
    if form is None and x is not None:
        form = rgcn_form(B, c_in, c_out, edge_type.numel(), n)
    basis = basis if basis.is_contiguous() else basis.contiguous()
    out = _RGCNPropagate.apply(x, basis, att, bias, graph, edge_type, edge_norm, plan, form)
    if root is not None:
        out = out + root if x is None else torch.addmm(out, x, root)
    return out


# ---------------------------------------------------------------------------
# DNAConv: per-edge attention over layer histories (csrc/mp_dna.hip)
# ---------------------------------------------------------------------------

def dna_ok(T, H, C):
    """Whether (T, H, C) lies inside the fused path's limits (mp_dna_ok)."""
    return bool(_lib.native().mp_dna_ok(int(T), int(H), int(C)))


def dna_max_layers(H, C):
    """The largest history length T the fused path takes for (heads, channels)
    (mp_dna_max_layers; 0 when it takes none; needs no GPU)."""
    return int(_lib.native().mp_dna_max_layers(int(H), int(C)))


def _dna_hist(t, what):
    """A [n, T, C] operand addressed in place: entry (t, c) of a row at t*C + c, any
    row stride >= T*C (a half of one fused K|V projection included)."""
    if t.dtype != torch.float32 or t.dim() != 3:
        raise TypeError("mi355_mp: %s must be float32 [n, T, C] (got %s %s)" % (what, t.dtype, tuple(t.shape)))
    n, T, C = t.shape
    if n and (t.stride(2) != 1 or t.stride(1) != C or t.stride(0) < T * C):
        t = t.contiguous()
    return t


def _dna_args(csr, q, k, v, norm, heads):
    q, k, v = _nnconv_rows(q, "q"), _dna_hist(k, "k"), _dna_hist(v, "v")
    n, T, C = k.shape
    if tuple(v.shape) != (n, T, C) or q.shape[1] != C:
        raise ValueError("mi355_mp: q %s, k %s and v %s disagree" % (tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    if norm is not None:
        if norm.dtype != torch.float32 or norm.dim() != 1:
            raise ValueError("mi355_mp: norm must be float32 [E] (got %s %s)" % (norm.dtype, tuple(norm.shape)))
        norm = norm.detach().contiguous()
    keep = (q, k, v, norm)
    args = (csr.struct("other"), q.data_ptr(), q.stride(0), _extent_bytes(q), k.data_ptr(), k.stride(0),
            _extent_bytes(k), v.data_ptr(), v.stride(0), _extent_bytes(v), _lib.ptr(norm),
            0 if norm is None else norm.numel())
    return keep, args, (T, int(heads), C)


def dna_split_chunk():
    """The schedule task size from which the DNA kernels walk tasks and split long
    rows (mp_dna_split_chunk; needs no GPU)."""
    return int(_lib.native().mp_dna_split_chunk())


def dna_target_tasks(n_rows, n_edges):
    """graph_for's target_tasks for a DNA layer: the schedule gets tasks of
    max(dna_split_chunk(), the default chunk) units, so the kernels walk tasks and
    split long rows on a graph of any size (None: the default schedule has such
    tasks already, and the layer shares the graph other layers build)."""
    from .graph import auto_chunk
    want = dna_split_chunk()
    if auto_chunk(n_rows, n_edges) >= want:
        return None
    return max((int(n_rows) + int(n_edges)) // want, 1)


def _dna_ws(nat, csr, slot_floats, dev):
    """(keep-alive tensor, pointer, bytes) of one call's slab (mp_dna_workspace);
    (None, None, 0) for a CSR the kernels walk by rows, which takes none."""
    n = nat.mp_dna_workspace(csr.struct("other"), int(slot_floats))
    if n <= nat.mp_dna_workspace(None, int(slot_floats)):      # the layout's minimum: no slab
        return None, None, 0
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    return ws, ws.data_ptr(), n


def _dna_drop(p, seed):
    p = float(p)
    return (int(seed or 0) & 0xFFFFFFFFFFFFFFFF, p)


def dna_aggregate(csr, q, k, v, norm, heads, p=0.0, seed=0, out=None, want_lse=False):
    """out[i, h] = sum over the slots (j -> i) of row i of norm[eid] * sum_t a_t v[j, t, h],
    a = the restricted softmax over t of <q[i, h], k[j, t, h]> / sqrt(d), after
    attention dropout (p, seed) when p > 0 (mp_dna_aggregate_f32).  q [n_rows, C],
    k, v [n_cols, T, C], norm fp32 [E] in edge order or None.  Returns out, or
    (out, lse [E, H]) with want_lse.  No autograd."""
    nat = _lib.native()
    keep, args, (T, H, C) = _dna_args(csr, q, k, v, norm, heads)
    dev = keep[0].device
    if out is None:
        out = torch.empty((csr.n_rows, C), dtype=torch.float32, device=dev)
    n_ids = max(int(getattr(csr, "n_ids", 0) or 0), csr.n_edges)
    lse = torch.empty((n_ids, H), dtype=torch.float32, device=dev) if want_lse else None
    ws, ws_ptr, ws_bytes = _dna_ws(nat, csr, C, dev)
    _count_call(nat, "mp_dna_aggregate_f32", *args, T, H, C, *_dna_drop(p, seed), out.data_ptr(), out.stride(0),
                _extent_bytes(out), _lib.ptr(lse), _lib.nbytes(lse), ws_ptr, ws_bytes, _lib.stream_ptr(dev))
    return (out, lse) if want_lse else out


def dna_backward_dst(csr, q, k, v, norm, gout, lse, heads, p=0.0, seed=0, out=None):
    """d q [n_rows, C] of dna_aggregate over the same destination CSR, a recomputed
    from lse (mp_dna_backward_dst_f32).  No autograd."""
    nat = _lib.native()
    keep, args, (T, H, C) = _dna_args(csr, q, k, v, norm, heads)
    gout = _nnconv_rows(gout, "gout")
    dev = gout.device
    if out is None:
        out = torch.empty((csr.n_rows, C), dtype=torch.float32, device=dev)
    ws, ws_ptr, ws_bytes = _dna_ws(nat, csr, C, dev)
    _count_call(nat, "mp_dna_backward_dst_f32", *args, gout.data_ptr(), gout.stride(0), _extent_bytes(gout),
                lse.data_ptr(), _lib.nbytes(lse), T, H, C, *_dna_drop(p, seed), out.data_ptr(), out.stride(0),
                _extent_bytes(out), ws_ptr, ws_bytes, _lib.stream_ptr(dev))
    return out


def dna_backward_src(csr, q, k, v, norm, gout, lse, heads, p=0.0, seed=0, dk=None, dv=None):
    """(d k, d v) [n_rows, T, C] of dna_aggregate over the SOURCE-keyed CSR (rows =
    sources: k, v; columns = destinations: q, gout) (mp_dna_backward_src_f32).
    No autograd."""
    nat = _lib.native()
    keep, args, (T, H, C) = _dna_args(csr, q, k, v, norm, heads)
    gout = _nnconv_rows(gout, "gout")
    dev = gout.device
    if dk is None:
        dk = torch.empty((csr.n_rows, T, C), dtype=torch.float32, device=dev)
    if dv is None:
        dv = torch.empty((csr.n_rows, T, C), dtype=torch.float32, device=dev)
    for t, what in ((dk, "dk"), (dv, "dv")):
        if t.dtype != torch.float32 or tuple(t.shape) != (csr.n_rows, T, C) or \
                (t.numel() and (t.stride(2) != 1 or t.stride(1) != C or t.stride(0) < T * C)):
            raise ValueError("mi355_mp: %s must be float32 [%d, %d, %d] with rows of T*C floats" % (what, csr.n_rows, T, C))
    ws, ws_ptr, ws_bytes = _dna_ws(nat, csr, 2 * T * C, dev)
    _count_call(nat, "mp_dna_backward_src_f32", *args, gout.data_ptr(), gout.stride(0), _extent_bytes(gout),
                lse.data_ptr(), _lib.nbytes(lse), T, H, C, *_dna_drop(p, seed), dk.data_ptr(), dk.stride(0),
                _extent_bytes(dk), dv.data_ptr(), dv.stride(0), _extent_bytes(dv), ws_ptr, ws_bytes,
                _lib.stream_ptr(dev))
    return dk, dv


def dna_dropout_keep(graph, seed, p, H, T):
    """The attention-dropout keep mask [E, H, T] (bool, the graph's edge order) that
    the fused DNA kernels apply for (seed, p) (mp_dna_dropout_keep)."""
    nat = _lib.native()
    csr = graph.dst
    E = csr.n_edges
    dev = csr.rowptr.device
    keep = torch.empty((E, int(H), int(T)), dtype=torch.uint8, device=dev)
    _count_call(nat, "mp_dna_dropout_keep", int(seed) & 0xFFFFFFFFFFFFFFFF, float(p), int(H), int(T), E,
                _lib.ptr(keep) if keep.numel() else None, _lib.nbytes(keep), _lib.stream_ptr(dev))
    return keep.bool()


class _DNAPropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, graph, norm, heads, p, seed):
        train = any(ctx.needs_input_grad[:3])
        res = dna_aggregate(graph.dst, q, k, v, norm, heads, p, seed, want_lse=train)
        out, lse = res if train else (res, None)
        ctx.graph, ctx.heads, ctx.p, ctx.seed = graph, heads, p, seed
        # the cached Graph holds its edge_index weakly and builds the transposed CSR
        # on first use, in backward: keep the tensor alive until then
        ctx.save_for_backward(q, k, v, norm, lse, graph._edge_index())
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, norm, lse, _ = ctx.saved_tensors
        graph = ctx.graph
        g = g.contiguous()
        gq = gk = gv = None
        if ctx.needs_input_grad[0]:
            gq = dna_backward_dst(graph.dst, q, k, v, norm, g, lse, ctx.heads, ctx.p, ctx.seed)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gk, gv = dna_backward_src(graph.src, q, k, v, norm, g, lse, ctx.heads, ctx.p, ctx.seed)
            gk = gk if ctx.needs_input_grad[1] else None
            gv = gv if ctx.needs_input_grad[2] else None
        return gq, gk, gv, None, None, None, None, None


def dna_propagate(graph, q, k, v, norm, heads, p=0.0, seed=None):
    """out[i] = sum_{e = (j -> i)} norm[e] * attention(q[i], k[j], v[j]) per head

    DNAConv's propagate on node-level projections: q [N, C] = lin_q(x[:, -1]),
    k, v [N, T, C] = lin_k(x), lin_v(x) (two tensors, or the halves of one fused
    projection); one query per destination attends over the T keys of every
    in-neighbour under the restricted softmax (margin 0), the messages are scaled
    by norm (fp32 [E], no gradient, or None) and summed.  No [E, T, C] array is
    built; the only per-edge float array is lse [E, H], kept for the backward.
    p in (0, 1): attention dropout with the hash mask of dna_dropout_keep(graph,
    seed, p, heads, T); seed None draws one (dropout_seed).  Deterministic, native
    forward and backward: d q over the destination CSR, d k and d v over the
    source-keyed one; a launch is skipped when nothing needs its gradient."""
    _lib.require_device(q, k, v, norm)
    if k.dim() != 3 or q.dim() != 2:
        raise ValueError("mi355_mp: q must be [N, C] and k, v [N, T, C] (got %s, %s)" % (tuple(q.shape), tuple(k.shape)))
    n, T, C = k.shape
    heads, p = int(heads), float(p)
    if norm is not None and norm.requires_grad:
        raise NotImplementedError("mi355_mp: dna_propagate has no gradient with respect to norm")
    if not 0.0 <= p < 1.0:
        raise ValueError("mi355_mp: attention dropout p must lie in [0, 1) (got %r)" % (p,))
    if heads < 1 or C % heads != 0 or not dna_ok(T, heads, C):
        raise NotImplementedError("mi355_mp: outside the fused DNA path's limits: T = %d, heads = %d, channels = %d "
                                  "(largest T: %d)" % (T, heads, C, dna_max_layers(heads, C) if heads >= 1 else 0))
    if n != graph.n_src or n != graph.n_dst or q.shape[0] != n:
        raise ValueError("mi355_mp: %d nodes (q %d), the graph %d sources and %d destinations"
                         % (n, q.shape[0], graph.n_src, graph.n_dst))
    if norm is not None and norm.numel() != graph.dst.n_edges:
        raise ValueError("mi355_mp: norm has %d entries, the graph %d edges" % (norm.numel(), graph.dst.n_edges))
    if p > 0.0 and seed is None:
        seed = dropout_seed(q.device)
    return _DNAPropagate.apply(q, k, v, graph, norm, heads, p, 0 if p == 0.0 else int(seed))


# ---------------------------------------------------------------------------
# TopKPooling (PyG 1.4.3 nn.pool.topk_pool [U]; csrc/mp_pool.hip)
# ---------------------------------------------------------------------------

class BatchLayout(object):
    """A non-decreasing batch vector as segment starts: starts [G + 1] (device
    int64, starts[G] = n), G graphs, max_n = the largest graph, unsorted = the
    number of descents (0 for a usable batch)."""
    __slots__ = ("starts", "n_graphs", "max_n", "unsorted", "n")

    def __init__(self, starts, n_graphs, max_n, unsorted, n):
        self.starts, self.n_graphs, self.max_n, self.unsorted, self.n = starts, n_graphs, max_n, unsorted, n


def check_ratio(ratio):
    """ratio in (0, 1]: upstream indexes into the padding of its dense copy otherwise."""
    if not (0.0 < float(ratio) <= 1.0):
        raise ValueError("TopKPooling: ratio must lie in (0, 1] (got %r)" % (ratio,))
    return float(ratio)


def topk_path(n_g):
    """0 = one wave, 1 = one workgroup, 2 = sorted: how mp_topk_select_f32 ranks a
    graph of n_g nodes (mp_topk_path; needs no GPU)."""
    return int(_lib.native().mp_topk_path(int(n_g)))


def batch_layout(batch, n, device=None):
    """BatchLayout of `batch` ([n] int64 on the device, or None = one graph).
    One host read (graphs, largest graph and sortedness together); none for
    batch None."""
    nat = _lib.native()
    n = int(n)
    if batch is None:
        starts = torch.tensor([0, n], dtype=torch.int64).to(device)
        return BatchLayout(starts, 1, n, 0, n)
    _lib.require_device(batch)
    if batch.dtype != torch.int64 or batch.dim() != 1 or batch.shape[0] != n:
        raise ValueError("mi355_mp: batch must be int64 [%d] (got %s %s)" % (n, batch.dtype, tuple(batch.shape)))
    batch = batch.contiguous()
    dev = batch.device
    st = _lib.stream_ptr(dev)
    stats = torch.empty(3, dtype=torch.int64, device=dev)
    nat.mp_batch_stats(batch.data_ptr(), n, stats.data_ptr(), _lib.nbytes(stats), st)
    G, max_n, unsorted = stats.tolist()
    starts = torch.empty(G + 1, dtype=torch.int64, device=dev)
    nat.mp_batch_starts(batch.data_ptr(), n, G, starts.data_ptr(), _lib.nbytes(starts), st)
    return BatchLayout(starts, G, min(max_n, n), unsorted, n)


def _pool_rows(x, what):
    x = _f32_2d(x, what)
    if x.shape[1] < 1:
        raise ValueError("mi355_mp: %s needs at least one feature" % what)
    if x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


class _PoolScore(torch.autograd.Function):
    """score = f(<attn, w> / ||w||) (mp_pool_score_f32) and its backward
    (mp_pool_score_bwd_f32: g_attn rows, g_w through fixed-order partials)."""

    @staticmethod
    def forward(ctx, attn, weight, flags):
        nat = _lib.native()
        attn = _pool_rows(attn, "attn")
        w = weight.detach().reshape(-1).contiguous()
        n, F = attn.shape
        if w.dtype != torch.float32 or w.numel() != F:
            raise ValueError("mi355_mp: weight must be float32 with %d entries (got %s %s)"
                             % (F, weight.dtype, tuple(weight.shape)))
        score = torch.empty(n, dtype=torch.float32, device=attn.device)
        nat.mp_pool_score_f32(attn.data_ptr(), attn.stride(0), n, F, w.data_ptr(), flags, score.data_ptr(),
                              _lib.nbytes(score), _lib.stream_ptr(attn.device))
        ctx.flags = flags
        ctx.wshape = weight.shape
        ctx.save_for_backward(attn, w, score)
        return score

    @staticmethod
    def backward(ctx, g):
        nat = _lib.native()
        attn, w, score = ctx.saved_tensors
        n, F = attn.shape
        dev = attn.device
        g = g.contiguous()
        g_attn = torch.empty((n, F), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        g_w = torch.empty(F, dtype=torch.float32, device=dev)
        wsb = nat.mp_pool_score_bwd_workspace(n, F)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        nat.mp_pool_score_bwd_f32(attn.data_ptr(), attn.stride(0), n, F, w.data_ptr(), ctx.flags, score.data_ptr(),
                                  g.data_ptr(), _lib.ptr(g_attn), F, g_w.data_ptr(), _lib.nbytes(g_w), ws.data_ptr(),
                                  wsb, _lib.stream_ptr(dev))
        return g_attn, (g_w.view(ctx.wshape) if ctx.needs_input_grad[1] else None), None


def pool_score(attn, weight, tanh=True, raw=False):
    """score [n] = f(<attn[i], w> / ||w||_2), f = tanh or the identity; raw: the
    bare projection <attn[i], w> (the min_score path).  Differentiable in attn
    and weight; ||w|| is computed on the device."""
    _lib.require_device(attn, weight)
    flags = (_lib.MP_POOL_SCORE_TANH if tanh else 0) | (_lib.MP_POOL_SCORE_RAW if raw else 0)
    return _PoolScore.apply(attn, weight, flags)


def topk_counts(starts, ratio, max_n=None):
    """(out_starts [G + 1], counts [4]) of mp_topk_counts: the exclusive scan of
    the device's k_g = ceil(fl32(ratio * fl32(n_g))) and K; no host read."""
    _lib.require_device(starts)
    G = starts.numel() - 1
    out_starts = torch.empty(G + 1, dtype=torch.int64, device=starts.device)
    counts = torch.zeros(4, dtype=torch.int64, device=starts.device)
    _lib.native().mp_topk_counts(starts.data_ptr(), G, check_ratio(ratio), (1 << 62) if max_n is None else int(max_n),
                                 out_starts.data_ptr(), _lib.nbytes(out_starts), counts.data_ptr(),
                                 _lib.stream_ptr(starts.device))
    return out_starts, counts


class PoolSelection(object):
    """What a select leaves on the device: perm (sized n, its first K entries
    valid), out_starts [G + 1] (None on the min_score path), inv [n] and counts
    (int64[4]: K, then filter_adj's kept edges and bad edge ends)."""
    __slots__ = ("perm", "out_starts", "inv", "counts")

    def __init__(self, perm, out_starts, inv, counts):
        self.perm, self.out_starts, self.inv, self.counts = perm, out_starts, inv, counts


def topk_select(score, ratio, layout):
    """Per-graph top-k of score [n] (mp_topk_select_f32): ceil(ratio * n_g) nodes
    of every graph by descending score, equal scores by ascending index.  No
    host read: K stays in counts[0]."""
    _lib.require_device(score)
    nat = _lib.native()
    ratio = check_ratio(ratio)
    score = score.detach()
    if score.dtype != torch.float32 or score.dim() != 1 or score.shape[0] != layout.n:
        raise ValueError("mi355_mp: score must be float32 [%d] (got %s %s)" % (layout.n, score.dtype, tuple(score.shape)))
    score = score.contiguous()
    dev = score.device
    n, G = layout.n, layout.n_graphs
    perm = torch.empty(n, dtype=torch.int64, device=dev)
    inv = torch.empty(n, dtype=torch.int64, device=dev)
    out_starts = torch.empty(G + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    wsb = nat.mp_topk_workspace(n, G, layout.max_n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    nat.mp_topk_select_f32(score.data_ptr(), n, layout.starts.data_ptr(), G, layout.max_n, ratio, perm.data_ptr(),
                           _lib.nbytes(perm), out_starts.data_ptr(), _lib.nbytes(out_starts), inv.data_ptr(),
                           _lib.nbytes(inv), counts.data_ptr(), ws.data_ptr(), wsb, _lib.stream_ptr(dev))
    return PoolSelection(perm, out_starts, inv, counts)


def pool_compact(keep, counts=None):
    """(pos, counts): pos[:counts[0]] = the positions with keep != 0 in ascending
    order (mp_pool_compact; pos is sized n).  No host read."""
    _lib.require_device(keep)
    nat = _lib.native()
    keep = keep.to(torch.uint8).contiguous()
    n = keep.numel()
    dev = keep.device
    pos = torch.empty(n, dtype=torch.int64, device=dev)
    if counts is None:
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
    wsb = nat.mp_pool_compact_workspace(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    nat.mp_pool_compact(keep.data_ptr(), n, pos.data_ptr(), _lib.nbytes(pos), counts.data_ptr(), ws.data_ptr(), wsb,
                        _lib.stream_ptr(dev))
    return pos, counts


def pool_inverse(perm, n, k_dev=None):
    """inv [n]: inv[perm[r]] = r, -1 elsewhere (mp_pool_inverse); k_dev: a device
    count bounding r when the host does not know it yet."""
    _lib.require_device(perm)
    perm = perm.to(torch.int64).contiguous()
    inv = torch.empty(int(n), dtype=torch.int64, device=perm.device)
    _lib.native().mp_pool_inverse(perm.data_ptr(), min(perm.numel(), int(n)), _lib.ptr(k_dev), int(n), inv.data_ptr(),
                                  _lib.nbytes(inv), _lib.stream_ptr(perm.device))
    return inv


def select_min_score(score, min_score, batch, layout, tol=1e-7):
    """upstream's min_score branch of topk: the nodes with
    score > min(max_g(score) - tol, min_score), in ascending node order.  The
    segment maximum and its gather are the engine's existing ops; the ordered
    compaction and the inverse map are mp_pool_compact / mp_pool_inverse."""
    _lib.require_device(score)
    score = score.detach()
    n = layout.n
    if batch is None:
        batch = torch.zeros(n, dtype=torch.int64, device=score.device)
    mx, _ = segment_reduce(score.view(-1, 1), batch, layout.n_graphs, "max")
    thr = (index_select_rows(mx, batch).view(-1) - tol).clamp(max=min_score)
    pos, counts = pool_compact(score > thr)
    inv = pool_inverse(pos, n, counts)
    return PoolSelection(pos, None, inv, counts)


def pool_filter_adj(edge_index, sel, n):
    """Launch filter_adj against sel.inv (mp_pool_filter_adj): returns (out [2, E],
    pos [E]) sized at their upper bound; sel.counts[1] = kept edges, [2] = edge
    ends outside [0, n).  No host read."""
    _lib.require_device(edge_index)
    nat = _lib.native()
    dev = edge_index.device
    E = int(edge_index.shape[1])
    row = edge_index[0].to(torch.int64).contiguous()
    col = edge_index[1].to(torch.int64).contiguous()
    out = torch.empty((2, E), dtype=torch.int64, device=dev)
    pos = torch.empty(E, dtype=torch.int64, device=dev)
    wsb = nat.mp_pool_filter_workspace(E)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    nat.mp_pool_filter_adj(row.data_ptr(), col.data_ptr(), E, sel.inv.data_ptr(), int(n), out[0].data_ptr(),
                           out[1].data_ptr(), pos.data_ptr(), E * 8, sel.counts.data_ptr(), ws.data_ptr(), wsb,
                           _lib.stream_ptr(dev))
    return out, pos


def pool_read_counts(sel, n):
    """The one host read after select and filter_adj: (K, kept edges).  Raises
    IndexError when an edge end lay outside [0, n), as upstream's mask[row] does."""
    K, kept, bad, _ = sel.counts.tolist()
    if K < 0:
        raise RuntimeError("mi355_mp: a graph is larger than the batch layout's max_n")
    if bad:
        raise IndexError("filter_adj: %d edge ends lie outside [0, %d)" % (bad, n))
    return K, kept


class _PoolGate(torch.autograd.Function):
    """x_out = multiplier * (x[perm] * score[perm]), score_out = score[perm],
    batch_out = batch[perm] (mp_pool_gate_f32); backward: one pass over all n
    nodes through inv (mp_pool_gate_bwd_f32), zeros for dropped nodes."""

    @staticmethod
    def forward(ctx, x, score, perm, inv, batch, multiplier):
        nat = _lib.native()
        x = _pool_rows(x, "x")
        score = score.contiguous()
        n, F = x.shape
        k = perm.numel()
        dev = x.device
        x_out = torch.empty((k, F), dtype=torch.float32, device=dev)
        score_out = torch.empty(k, dtype=torch.float32, device=dev)
        batch_out = torch.empty(k, dtype=torch.int64, device=dev)
        nat.mp_pool_gate_f32(x.data_ptr(), x.stride(0), score.data_ptr(), _lib.ptr(batch), perm.data_ptr(), k, n, F,
                             float(multiplier), x_out.data_ptr(), F, _lib.nbytes(x_out), batch_out.data_ptr(),
                             score_out.data_ptr(), _lib.stream_ptr(dev))
        ctx.k, ctx.multiplier = k, float(multiplier)
        ctx.save_for_backward(x, score, inv)
        ctx.mark_non_differentiable(batch_out)
        return x_out, score_out, batch_out

    @staticmethod
    def backward(ctx, g_y, g_t, _g_b=None):
        nat = _lib.native()
        x, score, inv = ctx.saved_tensors
        n, F = x.shape
        dev = x.device
        g_y = g_y.contiguous()
        g_t = g_t.contiguous()
        g_x = torch.empty((n, F), dtype=torch.float32, device=dev)
        g_s = torch.empty(n, dtype=torch.float32, device=dev)
        nat.mp_pool_gate_bwd_f32(g_y.data_ptr(), F, g_t.data_ptr(), x.data_ptr(), x.stride(0), score.data_ptr(),
                                 inv.data_ptr(), ctx.k, n, F, ctx.multiplier, g_x.data_ptr(), F, _lib.nbytes(g_x),
                                 g_s.data_ptr(), _lib.nbytes(g_s), _lib.stream_ptr(dev))
        return g_x, g_s, None, None, None, None


def pool_gate(x, score, perm, inv, batch=None, multiplier=1):
    """(x_out, score_out, batch_out) of the kept nodes perm (exact length K);
    differentiable in x and score.  inv: the inverse map of perm over x's rows."""
    _lib.require_device(x, score, perm, inv, batch)
    if score.dtype != torch.float32 or score.dim() != 1 or score.shape[0] != x.shape[0]:
        raise ValueError("mi355_mp: score must be float32 [%d]" % x.shape[0])
    if batch is not None:
        batch = batch.contiguous()
    return _PoolGate.apply(x, score, perm.contiguous(), inv, batch, multiplier)


class _GatherByPos(torch.autograd.Function):
    """attr[pos] for distinct positions pos; the gradient scatters back by pos."""

    @staticmethod
    def forward(ctx, attr, pos):
        ctx.n = attr.shape[0]
        ctx.save_for_backward(pos)
        return _gather_rows_bytes(attr, pos)

    @staticmethod
    def backward(ctx, g):
        (pos,) = ctx.saved_tensors
        out = torch.zeros((ctx.n,) + tuple(g.shape[1:]), dtype=g.dtype, device=g.device)
        out.index_copy_(0, pos, g)
        return out, None


def _gather_rows_bytes(attr, pos):
    """rows of any dtype whose elements are 2, 4 or 8 bytes wide (mp_gather_rows_any)."""
    width = 1
    for d in attr.shape[1:]:
        width *= int(d)
    flat = attr.reshape(attr.shape[0], width)            # not -1: ambiguous for a tensor of no rows (E = 0)
    if flat.stride(1) != 1 or flat.stride(0) < max(flat.shape[1], 1):
        flat = flat.contiguous()
    if flat.element_size() not in (2, 4, 8):
        raise TypeError("mi355_mp: edge_attr of dtype %s (%d-byte elements) is not supported"
                        % (attr.dtype, flat.element_size()))
    k, F = pos.numel(), flat.shape[1]
    out = torch.empty((k, F), dtype=attr.dtype, device=attr.device)
    if k and F:
        _lib.native().mp_gather_rows_any(flat.element_size(), flat.data_ptr(), flat.stride(0), pos.data_ptr(), k, F,
                                         out.data_ptr(), F, _lib.stream_ptr(attr.device))
    return out.view((k,) + tuple(attr.shape[1:]))


def pool_edge_attr(edge_attr, pos):
    """edge_attr[pos] for filter_adj's kept positions (any trailing shape)."""
    _lib.require_device(edge_attr, pos)
    pos = pos.contiguous()
    if edge_attr.requires_grad:
        return _GatherByPos.apply(edge_attr, pos)
    return _gather_rows_bytes(edge_attr, pos)


# ---------------------------------------------------------------------------
# Cluster pooling (PyG 1.4.3 nn.pool voxel_grid / max_pool / avg_pool [U]; csrc/mp_cluster.hip)
# ---------------------------------------------------------------------------

_layout_cache = _Cache()


def cached_batch_layout(batch, n, device=None):
    """batch_layout, cached on the batch tensor (identity + version counter, as
    index_range): one host read the first time a batch vector is seen."""
    if batch is None:
        return batch_layout(None, n, device)
    return _layout_cache.get(batch, ("layout", batch.data_ptr(), int(n)), lambda: batch_layout(batch, n, device))


def cached_batch_layout_for(batch, n, n_graphs, device=None):
    """The cached layout of a sorted batch, with trailing graphs without nodes up
    to n_graphs (a caller's size= beyond batch.max() + 1): starts padded with n,
    built once per (batch tensor, n_graphs) and cached like the layout itself.
    The plain layout when it is unsorted or holds n_graphs graphs or more."""
    layout = cached_batch_layout(batch, n, device)
    if layout.unsorted or layout.n_graphs >= n_graphs:
        return layout

    def extend():
        starts = torch.cat([layout.starts, layout.starts[-1:].expand(n_graphs - layout.n_graphs)])
        return BatchLayout(starts, n_graphs, layout.max_n, 0, layout.n)
    if batch is None:
        return extend()
    return _layout_cache.get(batch, ("layout_for", batch.data_ptr(), int(n), int(n_graphs)), extend)


_graphs_cache = _Cache()


def known_num_graphs(batch):
    """batch.max() + 1 when the host already knows it for this batch tensor (a
    cached layout, or note_num_graphs), else None.  Never reads."""
    if batch is None:
        return 1
    return _graphs_cache.get(batch, ("graphs", batch.data_ptr()), lambda: None)


def note_num_graphs(batch, n_graphs):
    """Record batch.max() + 1 of a batch vector the engine derived from one whose
    count it knew (a pooled batch keeps every graph that has a node)."""
    if batch is not None and n_graphs is not None:
        _graphs_cache.get(batch, ("graphs", batch.data_ptr()), lambda: int(n_graphs), valid=lambda v: v is not None)


def num_graphs(batch, n):
    """batch.max() + 1: known_num_graphs, else the (cached) batch layout's one read."""
    G = known_num_graphs(batch)
    if G is None:
        layout = cached_batch_layout(batch, n)
        # the layout counts graphs from the last entry: the maximum only for a sorted batch
        G = layout.n_graphs if not layout.unsorted else int(batch.max()) + 1
        note_num_graphs(batch, G)
    return G


def voxel_keys(pos, batch, size, start, end):
    """key [N] int64 of mp_voxel_keys_f32: pos [N, D] float32 (D <= 8), batch [N]
    int64 or None, size / start / end: float32 device tensors of D (+ 1 with a
    batch) entries.  No host read."""
    _lib.require_device(pos, batch, size, start, end)
    if pos.dtype != torch.float32:
        raise TypeError("mi355_mp: voxel_grid positions must be float32 (got %s)" % pos.dtype)
    pos = pos.detach()
    pos = pos.view(-1, 1) if pos.dim() == 1 else pos
    if pos.dim() != 2:
        raise ValueError("mi355_mp: pos must be [N] or [N, D]")
    if pos.stride(1) != 1 or pos.stride(0) < pos.shape[1]:
        pos = pos.contiguous()
    n, D = pos.shape
    Dt = D + (0 if batch is None else 1)
    if D > 8:
        raise ValueError("mi355_mp: voxel_grid takes at most 8 position columns (got %d)" % D)
    if batch is not None:
        if batch.dtype != torch.int64 or batch.dim() != 1 or batch.shape[0] != n:
            raise ValueError("mi355_mp: batch must be int64 [%d] (got %s %s)" % (n, batch.dtype, tuple(batch.shape)))
        batch = batch.contiguous()
    geo = []
    for name, t in (("size", size), ("start", start), ("end", end)):
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != Dt:
            raise ValueError("mi355_mp: %s must be float32 [%d] (got %s %s)" % (name, Dt, t.dtype, tuple(t.shape)))
        geo.append(t.contiguous())
    key = torch.empty(n, dtype=torch.int64, device=pos.device)
    _lib.native().mp_voxel_keys_f32(pos.data_ptr(), pos.stride(0), n, D, _lib.ptr(batch), geo[0].data_ptr(),
                                    geo[1].data_ptr(), geo[2].data_ptr(), key.data_ptr(), _lib.nbytes(key),
                                    _lib.stream_ptr(pos.device))
    return key


class ClusterSelection(object):
    """What mp_cluster_build leaves on the device: inv [n], the cluster CSR rowptr
    [n + 1] / member [n] (int32), perm (sized n, its first M entries valid) and
    counts (int64[4]: M, then pool_edges' output edges and bad edge ends).  M,
    n_edges_out: filled by cluster_read_counts."""
    __slots__ = ("inv", "rowptr", "member", "perm", "counts", "n", "M", "n_edges_out")

    def __init__(self, inv, rowptr, member, perm, counts, n):
        self.inv, self.rowptr, self.member, self.perm, self.counts, self.n = inv, rowptr, member, perm, counts, n
        self.M = self.n_edges_out = None

    def member_counts(self, M):
        """float32 [M, 1]: the number of nodes of every cluster."""
        return (self.rowptr[1:M + 1] - self.rowptr[:M]).to(torch.float32).view(-1, 1)


def cluster_build(key):
    """ClusterSelection of any int64 key vector (mp_cluster_build): one stable
    sort of (key, node index), the run heads and their scan.  No host read."""
    _lib.require_device(key)
    if key.dtype != torch.int64 or key.dim() != 1:
        raise ValueError("mi355_mp: cluster must be a 1-D int64 tensor (got %s %s)" % (key.dtype, tuple(key.shape)))
    nat = _lib.native()
    key = key.contiguous()
    n = key.numel()
    dev = key.device
    inv = torch.empty(n, dtype=torch.int64, device=dev)
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    member = torch.empty(n, dtype=torch.int32, device=dev)
    perm = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    wsb = nat.mp_cluster_build_workspace(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    nat.mp_cluster_build(key.data_ptr(), n, inv.data_ptr(), _lib.nbytes(inv), rowptr.data_ptr(), _lib.nbytes(rowptr),
                         member.data_ptr(), _lib.nbytes(member), perm.data_ptr(), _lib.nbytes(perm), counts.data_ptr(),
                         ws.data_ptr(), wsb, _lib.stream_ptr(dev))
    return ClusterSelection(inv, rowptr, member, perm, counts, n)


def cluster_read_counts(sel, n=None):
    """The one host read after everything has been enqueued: (M, E', bad edge
    ends), kept on sel.  Raises IndexError when pool_edges met an edge end
    outside [0, n), as upstream's cluster[edge_index] does."""
    if sel.M is None:
        M, kept, bad, _ = sel.counts.tolist()
        if bad:
            raise IndexError("pool_edge: %d edge ends lie outside [0, %d)" % (bad, sel.n if n is None else n))
        sel.M, sel.n_edges_out = M, kept
    return sel.M, sel.n_edges_out, 0


class _ClusterReduce(torch.autograd.Function):
    """mp_cluster_reduce_f32: (x_out, arg, pos_out, batch_out) at their upper bound
    of n rows, the first M valid.  Backward: the max routes every output gradient
    to its arg row (mp_scatter_arg_backward_f32); the means gather g / count by
    inv (gather_rows)."""

    @staticmethod
    def forward(ctx, x, pos, sel, reduce, batch, pyg_mask):
        nat = _lib.native()
        n = sel.n
        dev = sel.inv.device
        is_max = reduce == "max"
        F = Dp = 0
        x_out = arg = pos_out = batch_out = keep = None
        need_mask_grad = False
        if x is not None:
            x = _pool_rows(x, "x")
            F = x.shape[1]
            x_out = torch.empty((n, F), dtype=torch.float32, device=dev)
            arg = torch.empty((n, F), dtype=torch.int64, device=dev) if is_max else None
            need_mask_grad = pyg_mask and is_max and ctx.needs_input_grad[0]
        if pos is not None:
            pos = _pool_rows(pos, "pos")
            Dp = pos.shape[1]
            pos_out = torch.empty((n, Dp), dtype=torch.float32, device=dev)
        if batch is not None:
            batch_out = torch.empty(n, dtype=torch.int64, device=dev)
        flags = _lib.MP_FLAG_PYG_MASK if (pyg_mask and is_max and not need_mask_grad) else 0
        if n:
            nat.mp_cluster_reduce_f32(_lib.ptr(x), x.stride(0) if F else 0, F, _lib.MP_REDUCE[reduce], flags,
                                      sel.rowptr.data_ptr(), sel.member.data_ptr(), sel.counts.data_ptr(), n,
                                      _lib.ptr(x_out), F, _lib.nbytes(x_out), _lib.ptr(arg), _lib.nbytes(arg),
                                      _lib.ptr(pos), pos.stride(0) if Dp else 0, Dp, _lib.ptr(pos_out),
                                      _lib.nbytes(pos_out), _lib.ptr(batch), sel.perm.data_ptr(), _lib.ptr(batch_out),
                                      _lib.nbytes(batch_out), _lib.stream_ptr(dev))
        if need_mask_grad:
            keep = ~(x_out < -10000)
            x_out = x_out.masked_fill(~keep, 0.0)
        ctx.sel, ctx.is_max, ctx.F, ctx.Dp = sel, is_max, F, Dp
        ctx.save_for_backward(arg, keep)
        # an output follows its own input only: pooled positions of constant positions stay constant
        # (Cartesian pseudo-coordinates of them must not ask SplineConv for a pseudo gradient)
        const = [arg, batch_out, None if ctx.needs_input_grad[0] else x_out,
                 None if ctx.needs_input_grad[1] else pos_out]
        ctx.mark_non_differentiable(*[t for t in const if t is not None])
        return x_out, arg, pos_out, batch_out

    @staticmethod
    def backward(ctx, g_x, _g_arg, g_pos, _g_batch):
        sel = ctx.sel
        arg, keep = ctx.saved_tensors
        n = sel.n
        M = cluster_read_counts(sel)[0]
        gx = gp = None
        cnt = sel.member_counts(M)
        if ctx.F and ctx.needs_input_grad[0] and g_x is not None:
            g = g_x[:M]
            if keep is not None:
                g = g * keep[:M]
            g = g.contiguous()
            if ctx.is_max:
                gx = torch.zeros((n, ctx.F), dtype=torch.float32, device=g.device)
                _lib.native().mp_scatter_arg_backward_f32(g.data_ptr(), arg.data_ptr(), M, ctx.F, n, gx.data_ptr(),
                                                          ctx.F, _lib.stream_ptr(g.device))
            else:
                gx = gather_rows(g / cnt, sel.inv)
        if ctx.Dp and ctx.needs_input_grad[1] and g_pos is not None:
            gp = gather_rows(g_pos[:M] / cnt, sel.inv)
        return gx, gp, None, None, None, None


def cluster_reduce(sel, x=None, reduce="max", pos=None, batch=None, pyg_mask=True):
    """(x_out, arg, pos_out, batch_out) of the clusters of sel, each sized n with
    its first M rows valid (slice after cluster_read_counts): x_out = the max
    (arg = the winning node, the lowest index among equals; pyg_mask: out <
    -10000 := 0) or the mean of x over every cluster, pos_out = the mean of pos,
    batch_out = batch[perm].  float32 only; differentiable in x and pos.  No
    host read."""
    if reduce not in ("max", "mean"):
        raise ValueError("mi355_mp: cluster_reduce takes 'max' or 'mean' (got %r)" % (reduce,))
    _lib.require_device(sel.inv, x, pos, batch)
    for name, t in (("x", x), ("pos", pos)):
        if t is not None and t.shape[0] != sel.n:
            raise ValueError("mi355_mp: %s has %d rows, the clustering %d nodes" % (name, t.shape[0], sel.n))
    if batch is not None:
        if batch.dtype != torch.int64 or batch.dim() != 1 or batch.shape[0] != sel.n:
            raise ValueError("mi355_mp: batch must be int64 [%d]" % sel.n)
        batch = batch.contiguous()
    return _ClusterReduce.apply(x, pos, sel, reduce, batch, pyg_mask)


class EdgePooling(object):
    """What mp_cluster_edges leaves on the device: out [2, E] (first E' columns
    valid), edge_slot [E] (the output position of every original edge, -1 =
    dropped) and the duplicates of every output edge seg_ptr [E + 1] / seg_edge
    [E] (int32, ascending original position)."""
    __slots__ = ("out", "edge_slot", "seg_ptr", "seg_edge", "n_edges")

    def __init__(self, out, edge_slot, seg_ptr, seg_edge, n_edges):
        self.out, self.edge_slot, self.seg_ptr, self.seg_edge, self.n_edges = out, edge_slot, seg_ptr, seg_edge, n_edges


def pool_edges(edge_index, sel):
    """pool_edge's index side against sel.inv (mp_cluster_edges): relabel, drop
    the loops, sort the pairs and merge the duplicates; sel.counts[1] = output
    edges, [2] = edge ends outside [0, n).  No host read."""
    _lib.require_device(edge_index)
    nat = _lib.native()
    dev = edge_index.device
    E = int(edge_index.shape[1])
    row = edge_index[0].to(torch.int64).contiguous()
    col = edge_index[1].to(torch.int64).contiguous()
    out = torch.empty((2, E), dtype=torch.int64, device=dev)
    slot = torch.empty(E, dtype=torch.int64, device=dev)
    seg_ptr = torch.empty(E + 1, dtype=torch.int32, device=dev)
    seg_edge = torch.empty(E, dtype=torch.int32, device=dev)
    wsb = nat.mp_cluster_edges_workspace(E, sel.n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    nat.mp_cluster_edges(row.data_ptr(), col.data_ptr(), E, sel.inv.data_ptr(), sel.n, sel.counts.data_ptr(),
                         out[0].data_ptr(), out[1].data_ptr(), slot.data_ptr(), E * 8, seg_ptr.data_ptr(),
                         _lib.nbytes(seg_ptr), seg_edge.data_ptr(), _lib.nbytes(seg_edge), ws.data_ptr(), wsb,
                         _lib.stream_ptr(dev))
    sel.M = sel.n_edges_out = None
    return EdgePooling(out, slot, seg_ptr, seg_edge, E)


class _PoolEdgeAttr(torch.autograd.Function):
    """attr_out[k] = the sum of attr over the duplicates of output edge k in
    ascending original position (mp_cluster_edge_attr_f32), sized E rows; the
    backward hands every kept edge its output edge's gradient
    (mp_cluster_edge_attr_bwd_f32: a gather by edge_slot, 0 for a dropped edge)."""

    @staticmethod
    def forward(ctx, attr, ep, sel):
        flat = attr.reshape(attr.shape[0], -1)
        if flat.stride(1) != 1 or flat.stride(0) < max(flat.shape[1], 1):
            flat = flat.contiguous()
        E, A = flat.shape
        out = torch.empty((E, A), dtype=torch.float32, device=attr.device)
        if E and A:
            _lib.native().mp_cluster_edge_attr_f32(flat.data_ptr(), flat.stride(0), A, ep.seg_ptr.data_ptr(),
                                                   ep.seg_edge.data_ptr(), sel.counts.data_ptr(), E, out.data_ptr(), A,
                                                   _lib.nbytes(out), _lib.stream_ptr(attr.device))
        ctx.ep, ctx.sel, ctx.shape = ep, sel, attr.shape
        return out.view((E,) + tuple(attr.shape[1:]))

    @staticmethod
    def backward(ctx, g):
        E = ctx.shape[0]
        kept = cluster_read_counts(ctx.sel)[1]
        g = g.reshape(E, -1).contiguous()
        A = g.shape[1]
        ga = torch.empty((E, A), dtype=torch.float32, device=g.device)
        if E and A:
            _lib.native().mp_cluster_edge_attr_bwd_f32(g.data_ptr(), A, ctx.ep.edge_slot.data_ptr(), E, A, kept,
                                                       ga.data_ptr(), A, _lib.nbytes(ga), _lib.stream_ptr(g.device))
        return ga.view(ctx.shape), None, None


def pool_edge_attr_sum(edge_attr, ep, sel):
    """The coalesced edge attributes of pool_edges' output edges, sized E rows
    (slice to E' after cluster_read_counts).  float32 of any trailing shape;
    every other dtype is rejected (torch_sparse sums them with scatter_add, the
    native kernel is float32 only).  Differentiable.  No host read."""
    _lib.require_device(edge_attr)
    if edge_attr.dtype != torch.float32:
        raise TypeError("mi355_mp: pool_edge sums float32 edge attributes only (got %s)" % edge_attr.dtype)
    if edge_attr.shape[0] != ep.n_edges:
        raise ValueError("mi355_mp: edge_attr has %d rows, edge_index %d edges" % (edge_attr.shape[0], ep.n_edges))
    if edge_attr.numel() == 0:
        return edge_attr          # no edges (or no columns): the empty selection, as upstream's edge_attr[mask]
    return _PoolEdgeAttr.apply(edge_attr, ep, sel)


# Rounds enqueued per host read of graclus_match.  Measured (profiles/graclus_bench.json):
# the 64 x 75 superpixel-shaped batch takes 6 rounds unweighted and 9 with normalized-cut
# weights, the 2^20-node graph 10 and 13, so 8 covers them in one or two reads.  A round
# whose predecessor left nobody live is two launches that return at once; 16 per read
# saves the second read and pays for it in such launches (the same time within 1 %
# summed over the four cases), one round per read is 3 to 34 % slower.
GRACLUS_ROUNDS_PER_READ = 8


class GraclusMatching(object):
    """What graclus_match leaves: cluster [n] int64 on the device, and on the
    host the rounds the matching took, the device-to-host reads of the call and
    the launches the mp_graclus_* entry points enqueued (skipped rounds included)."""
    __slots__ = ("cluster", "rounds", "host_reads", "launches")

    def __init__(self, cluster, rounds, host_reads, launches):
        self.cluster, self.rounds, self.host_reads, self.launches = cluster, rounds, host_reads, launches


def _count_call(nat, name, *args):
    """The mp_graclus_* and point-set entry points return a count, or -(code): they
    are not among the status symbols native() wraps, so the sign is tested here."""
    rc = getattr(nat, name)(*args)
    if rc < 0:
        raise RuntimeError("%s failed (code %d): %s" % (name, -rc, nat.mp_last_error().decode(errors="replace")))
    return rc


_graclus_call = _count_call


def graclus_incidence(edge_index, n):
    """(row, col, rowptr, nbr, eid) of the node-sorted incidence list of the 2E
    directed entries of edge_index: mp_csr_build over cat(row, col) / cat(col, row),
    int32.  No host read: graclus_match reads the ends' range check with its counts."""
    nat = _lib.native()
    dev = edge_index.device
    E = int(edge_index.shape[1])
    row = edge_index[0].contiguous()
    col = edge_index[1].contiguous()
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    nbr = torch.empty(2 * E, dtype=torch.int32, device=dev)
    eid = torch.empty(2 * E, dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = nat.mp_csr_build_workspace(2 * E, n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    ends = torch.cat([row, col]) if E else None
    others = torch.cat([col, row]) if E else None
    nat.mp_csr_build(_lib.ptr(ends), _lib.ptr(others), 2 * E, n, n, rowptr.data_ptr(), _lib.ptr(nbr if E else None), _lib.ptr(eid if E else None),
                     bad.data_ptr(), ws.data_ptr(), wsb, _lib.stream_ptr(dev))
    return row, col, rowptr, nbr, eid


def graclus_match(edge_index, weight, n, seed=0, rounds_per_read=None):
    """The deterministic greedy matching of include/mi355_mp.h "Graclus" as a
    GraclusMatching: edge_index int64 [2, E], weight float32 [E] or None, n nodes.

    One node-sorted incidence list of the 2E directed entries (mp_csr_build),
    mp_graclus_init, then batches of rounds_per_read rounds (default
    GRACLUS_ROUNDS_PER_READ) with one host read of the counts after each, until a
    batch's last round leaves no node live: max(1, ceil(rounds / rounds_per_read))
    reads, none when there is no edge.  The incidence build's index check is read
    with the first batch.  An edge end outside [0, n) raises IndexError."""
    _lib.require_device(edge_index, weight)
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("mi355_mp: edge_index must be int64 [2, E] (got %s %s)"
                         % (edge_index.dtype, tuple(edge_index.shape)))
    n, E = int(n), int(edge_index.shape[1])
    if weight is not None:
        if weight.dtype != torch.float32:
            raise TypeError("mi355_mp: graclus weights must be float32 (got %s)" % weight.dtype)
        if weight.dim() != 1 or weight.shape[0] != E:
            raise ValueError("mi355_mp: weight must be [%d] (got %s)" % (E, tuple(weight.shape)))
        weight = weight.detach().contiguous()
    if n < 0 or n >= 1 << 30 or E >= 1 << 30:
        raise ValueError("mi355_mp: graclus takes fewer than 2^30 nodes and edges (got %d, %d)" % (n, E))
    if n == 0 and E:
        raise IndexError("graclus: %d edge ends lie outside [0, 0)" % (2 * E))
    R = int(GRACLUS_ROUNDS_PER_READ if rounds_per_read is None else rounds_per_read)
    if R < 1:
        raise ValueError("mi355_mp: rounds_per_read must be at least 1")
    nat = _lib.native()
    dev = edge_index.device
    st = _lib.stream_ptr(dev)
    row, col, rowptr, nbr, eid = graclus_incidence(edge_index, n)
    cluster = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    gwb = nat.mp_graclus_workspace(n, E)
    gws = torch.empty(gwb, dtype=torch.uint8, device=dev)
    tail = (_lib.ptr(cluster if n else None), _lib.nbytes(cluster), counts.data_ptr(), _lib.nbytes(counts),
            gws.data_ptr(), gwb, st)
    launches = _graclus_call(nat, "mp_graclus_init", _lib.ptr(row if E else None), _lib.ptr(col if E else None),
                             _lib.ptr(weight), _lib.nbytes(weight), E, n, int(seed) & _MASK64,
                             _lib.ptr(eid if E else None), _lib.nbytes(eid), *tail)
    rounds = reads = first = 0
    while E:
        launches += 2 * _graclus_call(nat, "mp_graclus_rounds", rowptr.data_ptr(), _lib.nbytes(rowptr), nbr.data_ptr(),
                                      _lib.nbytes(nbr), E, n, first, R, *tail)
        first += R
        got = counts.tolist()
        reads += 1
        if got[3]:
            raise IndexError("graclus: %d edges have an end outside [0, %d)" % (got[3] // 2, n))
        rounds = got[0]
        if got[1 + ((first - 1) & 1)] == 0:
            break
    return GraclusMatching(cluster, rounds, reads, launches)


# ---------------------------------------------------------------------------
# Point sets (PyG 1.4.3 nn.fps / nn.radius / nn.conv.PointConv [U]; csrc/mp_point.hip)
# ---------------------------------------------------------------------------

POINT_MAX_D = 8
_F32_MAX = 3.4028234663852886e38


def fps_path(n_g):
    """0 = one wave, 1 = one workgroup with the points in registers, 2 = one
    workgroup with m in the workspace: how mp_fps_f32 samples a graph of n_g
    points (mp_fps_path; needs no GPU)."""
    return int(_lib.native().mp_fps_path(int(n_g)))


def _point_rows(pos, what):
    """[n, D] float32 rows of a point tensor (1 <= D <= 8; a row stride is kept)."""
    if pos.dtype != torch.float32:
        raise TypeError("mi355_mp: %s must be float32 (got %s)" % (what, pos.dtype))
    pos = pos.view(-1, 1) if pos.dim() == 1 else pos
    if pos.dim() != 2:
        raise ValueError("mi355_mp: %s must be [N] or [N, D]" % what)
    if not 1 <= pos.shape[1] <= POINT_MAX_D:
        raise ValueError("mi355_mp: %s takes 1 to %d columns (got %d)" % (what, POINT_MAX_D, pos.shape[1]))
    if pos.stride(1) != 1 or pos.stride(0) < pos.shape[1]:
        pos = pos.contiguous()
    return pos


def _sorted_layout(batch, n, device, what):
    layout = cached_batch_layout(batch, n, device)
    if layout.unsorted:
        raise ValueError("mi355_mp: %s must be sorted (it descends %d times)" % (what, layout.unsorted))
    note_num_graphs(batch, layout.n_graphs)
    return layout


def fps(pos, batch=None, ratio=0.5, start=None):
    """Farthest point sampling (mp_fps_f32): idx int64 [K], grouped by graph in
    ascending order, within a graph in selection order; graph g keeps
    ceil(fl32(ratio * fl32(n_g))) points (the TopKPooling count).

    pos: float32 [n, D], D <= 8; batch: sorted int64 [n] or None; start: None
    (every graph starts at its first point) or a device int64 [G] of in-graph
    offsets.  A pure function of its arguments.  ValueError for an unsorted
    batch, D > 8 or a start outside [0, n_g).  One device-to-host read (K and
    the rejected starts), beyond the cached batch layout."""
    _lib.require_device(pos, batch, start)
    nat = _lib.native()
    ratio = check_ratio(ratio)
    pos = _point_rows(pos.detach(), "pos")
    n, D = pos.shape
    dev = pos.device
    layout = _sorted_layout(batch, n, dev, "batch")
    G = layout.n_graphs
    if start is not None:
        if start.dtype != torch.int64 or start.dim() != 1 or start.shape[0] != G:
            raise ValueError("mi355_mp: start must be int64 [%d] (got %s %s)" % (G, start.dtype, tuple(start.shape)))
        start = start.contiguous()
    out_starts, counts = topk_counts(layout.starts, ratio, layout.max_n)
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    wsb = nat.mp_fps_workspace(n, layout.max_n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _count_call(nat, "mp_fps_f32", _lib.ptr(pos if n else None), pos.stride(0), n, D, layout.starts.data_ptr(), G,
                layout.max_n, out_starts.data_ptr(), _lib.ptr(start), _lib.ptr(idx if n else None), _lib.nbytes(idx),
                counts.data_ptr(), _lib.nbytes(counts), ws.data_ptr(), wsb, _lib.stream_ptr(dev))
    K, bad = counts[:2].tolist()
    if bad:
        raise ValueError("fps: %d graphs have a start offset outside [0, n_g)" % bad)
    return idx[:K]


def fps_random_start(layout, generator=None):
    """start [G] for fps: floor(u * n_g) clamped to n_g - 1, u uniform on [0, 1)
    from torch's device generator.  No host read."""
    starts = layout.starts
    n_g = starts[1:] - starts[:-1]
    u = torch.rand(layout.n_graphs, device=starts.device, generator=generator)
    s = (u * n_g.to(torch.float32)).floor().to(torch.int64)
    return torch.minimum(s, n_g - 1).clamp_(min=0)


def radius_search(x, y, r, batch_x=None, batch_y=None, max_num_neighbors=32):
    """The fixed-radius neighbour search (mp_radius_search_f32 + mp_radius_fill):
    int64 [2, E], row 0 indices into y, row 1 into x, sorted by y then x; for every
    y the first max_num_neighbors points of x, in ascending index, of the same
    graph with d2(x_i, y) <= fl32(fl32(r) * fl32(r)).

    x [n_x, D], y [n_y, D] float32 (D <= 8); batch_x / batch_y: sorted int64 or
    both None.  ValueError for an unsorted batch, r negative or not finite,
    max_num_neighbors < 1, other widths.  One device-to-host read (E), beyond
    the cached batch layouts."""
    _lib.require_device(x, y, batch_x, batch_y)
    nat = _lib.native()
    r = float(r)
    if not (0.0 <= r <= _F32_MAX):
        raise ValueError("radius: r must be finite and not negative (got %r)" % (r,))
    cap = int(max_num_neighbors)
    if cap < 1:
        raise ValueError("radius: max_num_neighbors must be at least 1 (got %d)" % cap)
    if (batch_x is None) != (batch_y is None):
        raise ValueError("radius: batch_x and batch_y come together or not at all")
    x = _point_rows(x.detach(), "x")
    y = _point_rows(y.detach(), "y")
    if x.shape[1] != y.shape[1]:
        raise ValueError("radius: x has %d columns, y %d" % (x.shape[1], y.shape[1]))
    (n_x, D), n_y = x.shape, y.shape[0]
    dev = x.device
    lx = _sorted_layout(batch_x, n_x, dev, "batch_x")
    _sorted_layout(batch_y, n_y, dev, "batch_y")
    cap = min(cap, max(lx.max_n, 1))          # a query never finds more than its graph holds
    if n_y and cap >= (1 << 31) // n_y:
        raise ValueError("radius: n_y * max_num_neighbors = %d * %d is not below 2^31" % (n_y, cap))
    if batch_y is not None:
        batch_y = batch_y.contiguous()
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    wsb = nat.mp_radius_workspace(n_y, cap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    _count_call(nat, "mp_radius_search_f32", _lib.ptr(x if n_x else None), x.stride(0), n_x,
                _lib.ptr(y if n_y else None), y.stride(0), n_y, D, _lib.ptr(batch_y), lx.starts.data_ptr(), lx.n_graphs, r, cap, counts.data_ptr(),
                _lib.nbytes(counts), ws.data_ptr(), wsb, st)
    E = int(counts[0].item())
    out = torch.empty((2, E), dtype=torch.int64, device=dev)
    _count_call(nat, "mp_radius_fill", n_y, cap, E, _lib.ptr(out[0] if E else None), _lib.ptr(out[1] if E else None),
                E * 8, ws.data_ptr(), wsb, st)
    return out


class _PointEdgeFeatures(torch.autograd.Function):
    """[x_src[src] | pos_src[src] - pos_dst[dst]] in one pass
    (mp_point_edge_features_f32).  Backward: the row gather's backward by source
    for x_src and pos_src, the negated segment sum by destination for pos_dst --
    the engine's deterministic sums over the cached CSR of each index."""

    @staticmethod
    def forward(ctx, x_src, pos_src, pos_dst, src, dst):
        nat = _lib.native()
        F = 0 if x_src is None else x_src.shape[1]
        D = pos_src.shape[1]
        E = src.numel()
        dev = pos_src.device
        out = torch.empty((E, F + D), dtype=torch.float32, device=dev)
        _count_call(nat, "mp_point_edge_features_f32", _lib.ptr(x_src), 0 if x_src is None else x_src.stride(0), F,
                    pos_src.data_ptr(), pos_src.stride(0), pos_src.shape[0], pos_dst.data_ptr(), pos_dst.stride(0),
                    pos_dst.shape[0], D, src.data_ptr(), dst.data_ptr(), E, out.data_ptr(), F + D, _lib.nbytes(out),
                    _lib.stream_ptr(dev))
        ctx.F, ctx.n_src, ctx.n_dst = F, pos_src.shape[0], pos_dst.shape[0]
        ctx.save_for_backward(src, dst)
        return out

    @staticmethod
    def backward(ctx, g):
        src, dst = ctx.saved_tensors
        F = ctx.F
        g = g.contiguous()
        need_x = F > 0 and ctx.needs_input_grad[0]
        g_x = g_ps = g_pd = None
        if need_x or ctx.needs_input_grad[1]:
            by_src = csr_for_index(src, ctx.n_src)
            if need_x:
                g_x, _ = _aggregate(by_src, "eid", g[:, :F], None, "sum", 0, None)
            if ctx.needs_input_grad[1]:
                g_ps, _ = _aggregate(by_src, "eid", g[:, F:], None, "sum", 0, None)
        if ctx.needs_input_grad[2]:
            g_pd, _ = _aggregate(csr_for_index(dst, ctx.n_dst), "eid", g[:, F:], None, "sum", 0, None)
            g_pd = g_pd.neg_()
        return g_x, g_ps, g_pd, None, None


def point_edge_features(x_src, pos_src, pos_dst, src, dst):
    """PointConv's per-edge matrix [E, F + D]: out[e, :F] = x_src[src[e]] and
    out[e, F:] = pos_src[src[e]] - pos_dst[dst[e]]; x_src None means F = 0.
    Differentiable in x_src, pos_src and pos_dst; edges in any order.  An index
    outside its range raises IndexError (check_row_index: cached per index)."""
    _lib.require_device(x_src, pos_src, pos_dst, src, dst)
    pos_src = _point_rows(pos_src, "pos_src")
    pos_dst = _point_rows(pos_dst, "pos_dst")
    if pos_src.shape[1] != pos_dst.shape[1]:
        raise ValueError("mi355_mp: pos_src has %d columns, pos_dst %d" % (pos_src.shape[1], pos_dst.shape[1]))
    if x_src is not None:
        x_src = _f32_2d(x_src, "x_src")
        if x_src.shape[0] != pos_src.shape[0]:
            raise ValueError("mi355_mp: x_src has %d rows, pos_src %d" % (x_src.shape[0], pos_src.shape[0]))
        if x_src.shape[1] == 0:
            x_src = None
        elif x_src.stride(0) < x_src.shape[1]:
            x_src = x_src.contiguous()
    if src.dtype != torch.int64 or dst.dtype != torch.int64 or src.dim() != 1 or src.shape != dst.shape:
        raise ValueError("mi355_mp: src and dst must be int64 vectors of one length")
    if src.stride(0) != 1:
        src = src.contiguous()
    if dst.stride(0) != 1:
        dst = dst.contiguous()
    check_row_index(src, pos_src.shape[0], "point_edge_features")
    check_row_index(dst, pos_dst.shape[0], "point_edge_features")
    return _PointEdgeFeatures.apply(x_src, pos_src, pos_dst, src, dst)


# ---------------------------------------------------------------------------
# Nearest neighbours (PyG 1.4.3 nn.knn / nn.knn_graph / nn.nearest /
# nn.unpool.knn_interpolate [U]; csrc/mp_knn.hip)
# ---------------------------------------------------------------------------

KNN_MAX_K = 64          # one slot of the selection per lane (mp_knn_max_k)


def knn_max_d():
    """MP_KNN_MAX_D of the loaded library: the widest row knn searches (needs no GPU)."""
    return int(_lib.native().mp_knn_max_d())


def knn_path(D):
    """0 = query and candidates in registers (D <= 8), 1 = the general-width
    path: how mp_knn_search_f32 computes distances of width D (mp_knn_path;
    needs no GPU).  ValueError for a D outside [1, MP_KNN_MAX_D]."""
    p = int(_lib.native().mp_knn_path(int(D)))
    if p < 0:
        raise ValueError("knn: rows take 1 to %d columns (got %d)" % (knn_max_d(), int(D)))
    return p


def _knn_rows(pos, what):
    """[n, D] float32 rows of a point or feature tensor (1 <= D <= MP_KNN_MAX_D; a
    row stride is kept)."""
    if pos.dtype != torch.float32:
        raise TypeError("mi355_mp: %s must be float32 (got %s)" % (what, pos.dtype))
    pos = pos.view(-1, 1) if pos.dim() == 1 else pos
    if pos.dim() != 2:
        raise ValueError("mi355_mp: %s must be [N] or [N, D]" % what)
    if not 1 <= pos.shape[1] <= knn_max_d():
        raise ValueError("knn: %s takes 1 to %d columns (got %d)" % (what, knn_max_d(), pos.shape[1]))
    if pos.stride(1) != 1 or pos.stride(0) < pos.shape[1]:
        pos = pos.contiguous()
    return pos


_one_graph = {}


def _knn_layout(batch, n, device, what):
    """_sorted_layout; the layout of batch None (one graph of n rows) is kept per
    (device, n), so a repeated call copies nothing to the device."""
    if batch is not None:
        return _sorted_layout(batch, n, device, what)
    key = (str(device), int(n))
    layout = _one_graph.get(key)
    if layout is None:
        if len(_one_graph) >= 64:
            _one_graph.clear()
        layout = _one_graph[key] = batch_layout(None, n, device)
    return layout


class KnnSlab(object):
    """What the search leaves on the device: the workspace of mp_knn_search_f32
    (per query k neighbours, their d2 and a count, in ascending key; the scanned
    counts), counts (int64 [4], counts[0] = E), and n_edges when the host knows E
    without reading it (both batch vectors None), else None."""
    __slots__ = ("ws", "ws_bytes", "counts", "n_x", "n_y", "k", "n_edges", "device")

    def __init__(self, ws, ws_bytes, counts, n_x, n_y, k, n_edges, device):
        self.ws, self.ws_bytes, self.counts, self.n_x, self.n_y = ws, ws_bytes, counts, n_x, n_y
        self.k, self.n_edges, self.device = k, n_edges, device


def knn_slab(x, y, k, batch_x=None, batch_y=None, what="knn"):
    """mp_knn_search_f32: the k nearest rows of x for every row of y, left in a
    KnnSlab.  No device-to-host read beyond the cached batch layouts."""
    _lib.require_device(x, y, batch_x, batch_y)
    k = int(k)
    if k < 1:
        raise ValueError("%s: k must be at least 1 (got %d)" % (what, k))
    if k > KNN_MAX_K:
        raise ValueError("%s: k = %d is above the limit of %d neighbours (MP_KNN_MAX_K)" % (what, k, KNN_MAX_K))
    if (batch_x is None) != (batch_y is None):
        raise ValueError("%s: batch_x and batch_y come together or not at all" % what)
    x = _knn_rows(x.detach(), "x")
    y = _knn_rows(y.detach(), "y")
    if x.shape[1] != y.shape[1]:
        raise ValueError("%s: x has %d columns, y %d" % (what, x.shape[1], y.shape[1]))
    nat = _lib.native()
    (n_x, D), n_y = x.shape, y.shape[0]
    dev = x.device
    lx = _knn_layout(batch_x, n_x, dev, "batch_x")
    _knn_layout(batch_y, n_y, dev, "batch_y")
    k = min(k, max(lx.max_n, 1))                  # a query never finds more than its graph holds
    if n_y and k >= (1 << 31) // n_y:
        raise ValueError("%s: n_y * k = %d * %d is not below 2^31" % (what, n_y, k))
    if batch_y is not None:
        batch_y = batch_y.contiguous()
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    wsb = nat.mp_knn_workspace(n_y, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _count_call(nat, "mp_knn_search_f32", _lib.ptr(x if n_x else None), x.stride(0), n_x,
                _lib.ptr(y if n_y else None), y.stride(0), n_y, D, _lib.ptr(batch_y), lx.starts.data_ptr(),
                lx.n_graphs, k, counts.data_ptr(), _lib.nbytes(counts), ws.data_ptr(), wsb, _lib.stream_ptr(dev))
    n_edges = n_y * min(k, n_x) if batch_y is None else None
    return KnnSlab(ws, wsb, counts, n_x, n_y, k, n_edges, dev)


def knn_pairs(slab, weights=False):
    """mp_knn_fill: the slab compacted to int64 [2, E] (row 0 indexes y, row 1 x;
    sorted by y, within a y ascending in (d2, index)), and with `weights` the
    normalised interpolation weight w_t / W_j of every pair, float32 [E].  One
    device-to-host read (E) unless the slab knows it."""
    nat = _lib.native()
    E = slab.n_edges
    if E is None:
        E = slab.n_edges = int(slab.counts[0].item())
    dev = slab.device
    out = torch.empty((2, E), dtype=torch.int64, device=dev)
    w = torch.empty(E, dtype=torch.float32, device=dev) if weights else None
    _count_call(nat, "mp_knn_fill", slab.n_y, slab.k, E, _lib.ptr(out[0] if E else None),
                _lib.ptr(out[1] if E else None), E * 8, _lib.ptr(w if E else None), _lib.nbytes(w), slab.ws.data_ptr(),
                slab.ws_bytes, _lib.stream_ptr(dev))
    return (out, w) if weights else out


def knn_search(x, y, k, batch_x=None, batch_y=None):
    """The k-nearest-neighbour search (mp_knn_search_f32 + mp_knn_fill): int64
    [2, E], row 0 indices into y, row 1 into x; for every row of y the
    min(k, n_g) rows of x of the same graph smallest under (d2(x_i, y_j), i) --
    equal distances go to the lower index -- sorted by y and ascending in that
    key within a y.

    x [n_x, D], y [n_y, D] float32, 1 <= D <= MP_KNN_MAX_D (a row stride is kept);
    batch_x / batch_y: sorted int64 or both None; 1 <= k <= 64.  ValueError for an
    unsorted batch, a batch on one side only, k outside [1, 64], other widths.
    At most one device-to-host read (E), beyond the cached batch layouts; none
    when both batch vectors are None (then E = n_y * min(k, n_x))."""
    return knn_pairs(knn_slab(x, y, k, batch_x, batch_y))


class _KnnInterpolate(torch.autograd.Function):
    """out[j] = (sum_t w_t x[i_t]) / (sum_t w_t) straight from the slab
    (mp_knn_interpolate_f32): the forward never needs E.  Backward:
    d x[i] = sum_{(j, i)} (w_ji / W_j) g[j], the engine's deterministic weighted
    sum over a CSR of the compacted pairs keyed by the x index (one read of E, and
    the CSR's own)."""

    @staticmethod
    def forward(ctx, x, slab):
        nat = _lib.native()
        n_x, C = x.shape
        dev = x.device
        out = torch.empty((slab.n_y, C), dtype=torch.float32, device=dev)
        _count_call(nat, "mp_knn_interpolate_f32", _lib.ptr(x if n_x else None), x.stride(0), n_x, C, slab.n_y, slab.k,
                    slab.ws.data_ptr(), slab.ws_bytes, _lib.ptr(out if slab.n_y else None), C, _lib.nbytes(out),
                    _lib.stream_ptr(dev))
        ctx.slab, ctx.shape = slab, (n_x, C)
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        from .graph import CSR
        slab = ctx.slab
        n_x, C = ctx.shape
        pairs, w = knn_pairs(slab, weights=True)
        if pairs.shape[1] == 0:
            return torch.zeros((n_x, C), dtype=torch.float32, device=g.device), None
        g = _f32_2d(g, "grad")
        by_x = CSR(pairs[1], pairs[0], n_x, slab.n_y)
        gx, _ = _aggregate(by_x, "other", g, by_x.to_csr_order(w), "sum", 0, None)
        return gx, None


def knn_interpolate(x, pos_x, pos_y, batch_x=None, batch_y=None, k=3):
    """Inverse-squared-distance interpolation of x [n_x, C] from pos_x onto pos_y
    (upstream's nn.unpool.knn_interpolate): float32 [n_y, C],
    out[j] = (sum_t w_t x[i_t]) / (sum_t w_t) over the k nearest i_t of pos_y[j] in
    knn order, w_t = 1 / max(d2_t, 1e-16), both sums in fp32 in the order
    t = 0 .. c - 1.  A y whose graph holds no x gets zeros.  Differentiable in x
    only (upstream computes the weights under no_grad).  The forward makes no
    device-to-host read beyond the cached batch layouts."""
    _lib.require_device(x, pos_x, pos_y, batch_x, batch_y)
    x = _f32_2d(x, "x")
    if x.shape[1] < 1:
        raise ValueError("knn_interpolate: x must have at least one column")
    if x.stride(0) < x.shape[1]:
        x = x.contiguous()
    n_x = pos_x.shape[0]
    if x.shape[0] != n_x:
        raise ValueError("knn_interpolate: x has %d rows, pos_x %d" % (x.shape[0], n_x))
    slab = knn_slab(pos_x, pos_y, k, batch_x, batch_y, what="knn_interpolate")
    return _KnnInterpolate.apply(x, slab)


# ---------------------------------------------------------------------------
# Attention readout (PyG 1.4.3 nn.glob.Set2Set / GlobalAttention [U]; csrc/mp_glob.hip)
# ---------------------------------------------------------------------------

def readout_path(n_g, C):
    """0 = one wave, 1 = one workgroup, 2 = split into chunks: how the attention
    readout reduces a graph of n_g nodes and C channels (mp_readout_path; needs
    no GPU).  ValueError for C < 1."""
    p = int(_lib.native().mp_readout_path(int(n_g), int(C)))
    if p < 0:
        raise ValueError("readout_path: n_g = %d, C = %d (n_g >= 0 and C >= 1)" % (n_g, C))
    return p


def readout_chunk(C):
    """Nodes per chunk of a graph on path 2 (mp_readout_chunk; needs no GPU)."""
    c = int(_lib.native().mp_readout_chunk(int(C)))
    if c < 0:
        raise ValueError("readout_chunk: C = %d < 1" % C)
    return c


def _readout_ws(nat, layout, n, C, dev):
    wsb = nat.mp_readout_workspace(n, layout.n_graphs, layout.max_n, C)
    return torch.empty(wsb, dtype=torch.uint8, device=dev), wsb


class _AttentionReadout(torch.autograd.Function):
    """r_g = sum_n softmax_g(e)_n x_n with e = x . q[g] (q given) or e = score, in
    one pass (mp_attention_readout_f32); saves x, q, e, (m, den) and r, and the
    backward is one pass again (mp_attention_readout_bwd_f32).  Gradients nobody
    needs are not computed."""

    @staticmethod
    def forward(ctx, x, q, score, layout, out, col):
        nat = _lib.native()
        n, C = x.shape
        G = layout.n_graphs
        dev = x.device
        given = out is not None
        if not given:
            out = torch.empty((G, C), dtype=torch.float32, device=dev)
            col = 0
        r = out[:, col:col + C]
        q_out = out[:, :C] if (q is not None and col >= C) else None
        e = torch.empty(n, dtype=torch.float32, device=dev)
        stats = torch.empty((G, 2), dtype=torch.float32, device=dev)
        ws, wsb = _readout_ws(nat, layout, n, C, dev)
        nz, gz = n > 0, G > 0
        # the pointers select the mode; a score vector of no nodes has none, and is never read
        score_ptr = None if score is None else (score.data_ptr() if nz else stats.data_ptr())
        _count_call(nat, "mp_attention_readout_f32", _lib.ptr(x if nz else None), x.stride(0), n, C,
                    layout.starts.data_ptr(), G, layout.max_n, _lib.ptr(q), 0 if q is None else q.stride(0),
                    score_ptr, _lib.ptr(r if gz else None), out.stride(0), _strided_bytes(r),
                    _lib.ptr(q_out), 0 if q_out is None else _strided_bytes(q_out), _lib.ptr(e if nz else None),
                    _lib.nbytes(e), _lib.ptr(stats if gz else None), _lib.nbytes(stats), None, 0, ws.data_ptr(), wsb,
                    _lib.stream_ptr(dev))
        ctx.layout, ctx.query, ctx.col, ctx.q_copied = layout, q is not None, col, q_out is not None
        if given:
            ctx.mark_dirty(out)
        ctx.save_for_backward(x, q, e, stats, out)
        return out

    @staticmethod
    def backward(ctx, g_out):
        nat = _lib.native()
        x, q, e, stats, out = ctx.saved_tensors
        layout, col = ctx.layout, ctx.col
        n, C = x.shape
        G = layout.n_graphs
        dev = x.device
        r = out[:, col:col + C]
        dr = g_out[:, col:col + C]
        if dr.stride(1) != 1 or dr.stride(0) < C:                    # a broadcast gradient (out.sum(0)) has row stride 0
            dr = dr.contiguous()
        need_x, need_q, need_s = ctx.needs_input_grad[0], ctx.query and ctx.needs_input_grad[1], \
            (not ctx.query) and ctx.needs_input_grad[2]
        dx = torch.empty((n, C), dtype=torch.float32, device=dev) if need_x else None
        dq = torch.empty((G, C), dtype=torch.float32, device=dev) if need_q else None
        ds = torch.empty(n, dtype=torch.float32, device=dev) if need_s else None
        ws, wsb = _readout_ws(nat, layout, n, C, dev)
        nz, gz = n > 0, G > 0
        _count_call(nat, "mp_attention_readout_bwd_f32", _lib.ptr(dr if gz else None), dr.stride(0),
                    _lib.ptr(x if nz else None), x.stride(0), n, C, layout.starts.data_ptr(), G, layout.max_n,
                    _lib.ptr(q), 0 if q is None else q.stride(0), _lib.ptr(e if nz else None),
                    _lib.ptr(stats if gz else None), _lib.ptr(r if gz else None), r.stride(0),
                    _lib.ptr(dx if nz else None), C, _lib.nbytes(dx), _lib.ptr(dq if gz else None), C, _lib.nbytes(dq),
                    _lib.ptr(ds if nz else None), _lib.nbytes(ds), ws.data_ptr(), wsb, _lib.stream_ptr(dev))
        if ctx.q_copied and need_q:                                   # columns 0 .. C of out are q itself
            dq = dq + g_out[:, :C]
        return dx, dq, ds, None, None, None


def _strided_bytes(t):
    """Extent in bytes of the rows of a 2-D view from its first element on."""
    return 0 if t.shape[0] == 0 else ((t.shape[0] - 1) * t.stride(0) + t.shape[1]) * t.element_size()


def attention_readout(x, layout, q=None, score=None, out=None, col=0):
    """The softmax-weighted per-graph sum of x's rows (include/mi355_mp.h
    "Attention readout"): x float32 [n, C]; layout: the BatchLayout of a sorted
    batch vector (cached_batch_layout); exactly one of q float32 [G, C] (e = x .
    q[graph]) and score float32 [n] (e = score).  Returns r [G, C], or, with out
    (float32 [G, W], fresh memory) given, out itself with r written into its
    columns col .. col + C (out is modified in place); in query mode with col >=
    C the columns 0 .. C receive q (Set2Set's q_star = [q | r] with col = C, W
    = 2C).
    Differentiable in x and q or score.  Tensors must be on the GPU."""
    _lib.require_device(x, q, score, out, layout.starts)
    if (q is None) == (score is None):
        raise ValueError("mi355_mp: attention_readout takes exactly one of q and score")
    if layout.unsorted:
        raise ValueError("mi355_mp: batch must be sorted (it descends %d times)" % layout.unsorted)
    x = _f32_2d(x, "x")
    n, C = x.shape
    if C < 1:
        raise ValueError("mi355_mp: attention_readout needs at least one channel")
    if x.stride(0) < C:
        x = x.contiguous()
    if n != layout.n:
        raise ValueError("mi355_mp: x has %d rows, the batch layout %d" % (n, layout.n))
    G = layout.n_graphs
    if G == 0:
        return x.new_zeros((0, C if out is None else out.shape[1]))
    if q is not None:
        q = _f32_2d(q, "q")
        if q.shape != (G, C):
            raise ValueError("mi355_mp: q must be [%d, %d] (got %s)" % (G, C, tuple(q.shape)))
        if q.stride(0) < C:
            q = q.contiguous()
    else:
        if score.dtype != torch.float32 or score.numel() != n:
            raise ValueError("mi355_mp: score must be float32 with %d entries (got %s %s)"
                             % (n, score.dtype, tuple(score.shape)))
        score = score.reshape(-1).contiguous()
    if out is not None:
        if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != G or out.stride(1) != 1 \
                or col < 0 or col + C > out.shape[1] or out.stride(0) < out.shape[1]:
            raise ValueError("mi355_mp: out must be float32 [%d, >= %d] with unit column stride" % (G, col + C))
        if out.requires_grad:
            raise ValueError("mi355_mp: out is overwritten in place and must not require a gradient")
    return _AttentionReadout.apply(x, q, score, layout, out, int(col))


# ---------------------------------------------------------------------------
# The dense family (PyG 1.4.3 nn.dense, utils.to_dense_batch / to_dense_adj [U]; csrc/mp_dense.hip)
# ---------------------------------------------------------------------------

def diff_pool_path(N, C, F):
    """0 = one workgroup per graph (P, T and V in LDS), 1 = row tiles of the GEMM
    core with partials in the workspace: how mp_dense_diff_pool_f32 runs graphs
    of N nodes, C clusters and F features (mp_diff_pool_path; needs no GPU).
    ValueError unless all three are >= 1."""
    p = int(_lib.native().mp_diff_pool_path(int(N), int(C), int(F)))
    if p < 0:
        raise ValueError("diff_pool_path: N = %d, C = %d, F = %d (each >= 1)" % (N, C, F))
    return p


def _dense_3d(t, what, last=None):
    if t.dtype != torch.float32 or t.dim() != 3 or (last is not None and t.shape[2] != last):
        raise ValueError("mi355_mp: %s must be float32 [B, N, %s] (got %s %s)"
                         % (what, "*" if last is None else last, t.dtype, tuple(t.shape)))
    return t.contiguous()


def _dense_mask(mask, B, N):
    if mask is None:
        return None
    if mask.numel() != B * N:
        raise ValueError("mi355_mp: mask must hold [%d, %d] entries (got %s)" % (B, N, tuple(mask.shape)))
    return (mask.reshape(B, N) != 0).to(torch.uint8).contiguous()


class _DenseDiffPool(torch.autograd.Function):
    """(out, out_adj, link_loss, ent_loss) of mp_dense_diff_pool_f32; saves x and
    the forward's P, T, V and loss sums, so the backward
    (mp_dense_diff_pool_bwd_f32) never reads adj.  adj gets no gradient."""

    @staticmethod
    def forward(ctx, x, adj, s, mask):
        nat = _lib.native()
        B, N, F = x.shape
        C = s.shape[2]
        dev = x.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        out, out_adj, loss = new(B, C, F), new(B, C, C), new(4)
        P, T, V = new(B, N, C), new(B, N, C), new(B, N, C)
        wsb = nat.mp_diff_pool_workspace(B, N, C, F)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        _count_call(nat, "mp_dense_diff_pool_f32", x.data_ptr(), adj.data_ptr(), s.data_ptr(), _lib.ptr(mask), B, N, C,
                    F, out.data_ptr(), _lib.nbytes(out), out_adj.data_ptr(), _lib.nbytes(out_adj), loss.data_ptr(),
                    _lib.nbytes(loss), P.data_ptr(), _lib.nbytes(P), T.data_ptr(), _lib.nbytes(T), V.data_ptr(),
                    _lib.nbytes(V), ws.data_ptr(), wsb, _lib.stream_ptr(dev))
        ctx.save_for_backward(x, P, T, V, loss)
        ctx.mark_non_differentiable(P)
        return out, out_adj, loss[0], loss[1], P

    @staticmethod
    def backward(ctx, g_out, g_oa, g_link, g_ent, _g_p):
        nat = _lib.native()
        x, P, T, V, loss = ctx.saved_tensors
        B, N, F = x.shape
        C = P.shape[2]
        dev = x.device
        need_x, need_s = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        if not need_x and not need_s:
            return None, None, None, None
        g_out = None if g_out is None else g_out.contiguous()
        g_oa = None if g_oa is None else g_oa.contiguous()
        g_loss = None
        if g_link is not None or g_ent is not None:
            zero = loss.new_zeros(())
            g_loss = torch.stack([zero if g_link is None else g_link.reshape(()),
                                  zero if g_ent is None else g_ent.reshape(())]).contiguous()
        dx = torch.empty((B, N, F), dtype=torch.float32, device=dev) if need_x else None
        ds = torch.empty((B, N, C), dtype=torch.float32, device=dev)
        wsb = nat.mp_diff_pool_bwd_workspace(B, N, C, F)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        _count_call(nat, "mp_dense_diff_pool_bwd_f32", _lib.ptr(g_out), _lib.ptr(g_oa), _lib.ptr(g_loss), x.data_ptr(),
                    P.data_ptr(), T.data_ptr(), V.data_ptr(), loss.data_ptr(), B, N, C, F, _lib.ptr(dx),
                    _lib.nbytes(dx), ds.data_ptr(), _lib.nbytes(ds), ws.data_ptr(), wsb, _lib.stream_ptr(dev))
        return dx, None, ds if need_s else None, None


def dense_diff_pool(x, adj, s, mask=None, want_assignment=False):
    """The fused dense_diff_pool (include/mi355_mp.h "The dense family"): x [B, N,
    F], adj [B, N, N], s [B, N, C] float32 on the GPU, mask [B, N] (any dtype,
    non-zero = a node) or None.  Returns (out [B, C, F], out_adj [B, C, C],
    link_loss, ent_loss), and P = softmax(s) * mask as a fifth value with
    want_assignment.  Differentiable in x and s; adj must not require a gradient
    (the fused backward never forms one)."""
    _lib.require_device(x, adj, s, mask)
    if adj.requires_grad:
        raise ValueError("mi355_mp: the fused dense_diff_pool gives adj no gradient; adj.requires_grad is set")
    x = _dense_3d(x, "x")
    B, N, F = x.shape
    adj = _dense_3d(adj, "adj", N)
    s = _dense_3d(s, "s")
    C = s.shape[2]
    if adj.shape[:2] != (B, N) or s.shape[:2] != (B, N) or min(B, N, C, F) < 1:
        raise ValueError("mi355_mp: dense_diff_pool takes x [B, N, F], adj [B, N, N], s [B, N, C], all >= 1 (got %s, "
                         "%s, %s)" % (tuple(x.shape), tuple(adj.shape), tuple(s.shape)))
    res = _DenseDiffPool.apply(x, adj, s, _dense_mask(mask, B, N))
    return res if want_assignment else res[:4]


class _DenseMeanAgg(torch.autograd.Function):
    """mp_dense_mean_agg_f32 and, as its backward for x, the same call over the
    transposed adjacency with the saved degrees."""

    @staticmethod
    def forward(ctx, x, adj, add_loop):
        nat = _lib.native()
        B, N, F = x.shape
        dev = x.device
        out = torch.empty((B, N, F), dtype=torch.float32, device=dev)
        deg = torch.empty((B, N), dtype=torch.float32, device=dev)
        _count_call(nat, "mp_dense_mean_agg_f32", adj.data_ptr(), x.data_ptr(), B, N, F, int(add_loop), 0, None,
                    out.data_ptr(), _lib.nbytes(out), deg.data_ptr(), _lib.nbytes(deg), _lib.stream_ptr(dev))
        ctx.add_loop = int(add_loop)
        ctx.save_for_backward(adj, deg)
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        nat = _lib.native()
        adj, deg = ctx.saved_tensors
        g = g.contiguous()
        B, N, F = g.shape
        dx = torch.empty_like(g)
        _count_call(nat, "mp_dense_mean_agg_f32", adj.data_ptr(), g.data_ptr(), B, N, F, ctx.add_loop, 1,
                    deg.data_ptr(), dx.data_ptr(), _lib.nbytes(dx), None, 0, _lib.stream_ptr(g.device))
        return dx, None, None


def dense_mean_agg(x, adj, add_loop=True):
    """agg[b, i] = sum_j A^_ij x[b, j] / max(sum_j A^_ij, 1) with A^ = adj, its
    diagonal read as 1 when add_loop (adj is not copied): x [B, N, F], adj [B, N,
    N] float32 on the GPU.  Differentiable in x; adj must not require a gradient."""
    _lib.require_device(x, adj)
    if adj.requires_grad:
        raise ValueError("mi355_mp: the fused dense_mean_agg gives adj no gradient; adj.requires_grad is set")
    x = _dense_3d(x, "x")
    B, N, F = x.shape
    adj = _dense_3d(adj, "adj", N)
    if adj.shape[:2] != (B, N) or min(B, N, F) < 1:
        raise ValueError("mi355_mp: dense_mean_agg takes x [B, N, F] and adj [B, N, N], all >= 1 (got %s, %s)"
                         % (tuple(x.shape), tuple(adj.shape)))
    return _DenseMeanAgg.apply(x, adj, bool(add_loop))


class _ToDenseBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, layout, fill):
        nat = _lib.native()
        n, F = x.shape
        B, Nmax = layout.n_graphs, layout.max_n
        dev = x.device
        out = torch.empty((B, Nmax, F), dtype=torch.float32, device=dev)
        mask = torch.empty((B, Nmax), dtype=torch.uint8, device=dev)
        _count_call(nat, "mp_to_dense_batch_f32", _lib.ptr(x if n else None), n, F, layout.starts.data_ptr(), B, Nmax,
                    float(fill), _lib.ptr(out if out.numel() else None), _lib.nbytes(out),
                    _lib.ptr(mask if mask.numel() else None), _lib.nbytes(mask), _lib.stream_ptr(dev))
        ctx.layout, ctx.n = layout, n
        mask = mask.bool()
        ctx.mark_non_differentiable(mask)
        return out, mask

    @staticmethod
    def backward(ctx, g, _g_mask):
        nat = _lib.native()
        layout, n = ctx.layout, ctx.n
        g = g.contiguous()
        F = g.shape[2]
        dx = torch.empty((n, F), dtype=torch.float32, device=g.device)
        _count_call(nat, "mp_to_dense_batch_bwd_f32", _lib.ptr(g if g.numel() else None), n, F,
                    layout.starts.data_ptr(), layout.n_graphs, layout.max_n, _lib.ptr(dx if n else None),
                    _lib.nbytes(dx), _lib.stream_ptr(g.device))
        return dx, None, None


def to_dense_batch(x, layout, fill_value=0.0):
    """(dense [B, max_n, F], mask [B, max_n] bool) of the rows x [n, F] (float32, on
    the GPU) under the BatchLayout of a sorted batch vector (mp_to_dense_batch_f32);
    padding rows hold fill_value.  Differentiable in x (a row gather)."""
    _lib.require_device(x, layout.starts)
    if layout.unsorted:
        raise ValueError("mi355_mp: batch must be sorted (it descends %d times)" % layout.unsorted)
    x = _f32_2d(x, "x")
    if x.shape[0] != layout.n or x.shape[1] < 1:
        raise ValueError("mi355_mp: x must be [%d, >= 1] for this batch layout (got %s)" % (layout.n, tuple(x.shape)))
    return _ToDenseBatch.apply(x.contiguous(), layout, float(fill_value))


def to_dense_adj(edge_index, layout, batch=None, edge_attr=None):
    """[B, max_n, max_n] float32 with 1 per edge, or [B, max_n, max_n, D] holding
    edge_attr [E, D] (float32; of several edges of one cell the last in edge
    order wins), under the BatchLayout of the sorted batch vector `batch` (None =
    one graph): mp_to_dense_adj_f32.  Not differentiable."""
    nat = _lib.native()
    _lib.require_device(edge_index, layout.starts, batch, edge_attr)
    if layout.unsorted:
        raise ValueError("mi355_mp: batch must be sorted (it descends %d times)" % layout.unsorted)
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("mi355_mp: edge_index must be int64 [2, E] (got %s %s)"
                         % (edge_index.dtype, tuple(edge_index.shape)))
    B, Nmax, n = layout.n_graphs, layout.max_n, layout.n
    if batch is None and B > 1:
        raise ValueError("mi355_mp: to_dense_adj needs the batch vector of a layout of %d graphs" % B)
    row, col = edge_index[0].contiguous(), edge_index[1].contiguous()
    E = row.shape[0]
    D = 0
    if edge_attr is not None:
        if edge_attr.dtype != torch.float32 or edge_attr.dim() != 2 or edge_attr.shape[0] != E \
                or edge_attr.shape[1] < 1:
            raise ValueError("mi355_mp: edge_attr must be float32 [%d, >= 1] (got %s %s)"
                             % (E, edge_attr.dtype, tuple(edge_attr.shape)))
        edge_attr = edge_attr.detach().contiguous()
        D = edge_attr.shape[1]
    dev = edge_index.device
    out = torch.empty((B, Nmax, Nmax) + ((D,) if D else ()), dtype=torch.float32, device=dev)
    wsb = nat.mp_to_dense_adj_workspace(B, Nmax, D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _count_call(nat, "mp_to_dense_adj_f32", _lib.ptr(row if E else None), _lib.ptr(col if E else None), E,
                _lib.ptr(edge_attr), D, _lib.ptr(None if batch is None else batch.contiguous()), n,
                layout.starts.data_ptr(), B, Nmax, _lib.ptr(out if out.numel() else None), _lib.nbytes(out),
                ws.data_ptr(), wsb, _lib.stream_ptr(dev))
    return out


# ---------------------------------------------------------------------------
# link prediction: edge scores, the reconstruction loss, negative sampling
# (csrc/mp_link.hip; PyG 1.4.x nn.models.autoencoder, utils.negative_sampling [U])
# ---------------------------------------------------------------------------

def link_lanes(C, vec4=True):
    """Lanes that serve one edge of a z of C columns (mp_link_lanes): the power of
    two covering C / 4 lanes of 16-byte loads, at most 16 (vec4 and C % 4 == 0), or
    C scalar lanes, at most 64."""
    return int(_count_call(_lib.load(), "mp_link_lanes", int(C), int(bool(vec4))))


def _link_args(z, edge_index, what, trusted=False):
    """(z, row, col) of a scoring call: z float32 [N, C >= 1] with unit column
    stride, edge_index int64 [2, E] within [0, N) (check_row_index: one read the
    first time a tensor is seen; trusted: the sampler's own output)."""
    _lib.require_device(z, edge_index)
    z = _f32_2d(z, "z")
    if z.shape[1] < 1:
        raise ValueError("mi355_mp: z must have at least one column (got %s)" % (tuple(z.shape),))
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("mi355_mp: edge_index must be int64 [2, E] (got %s %s)"
                         % (edge_index.dtype, tuple(edge_index.shape)))
    if not trusted:
        check_row_index(edge_index, z.shape[0], what)
    return z, edge_index[0].contiguous(), edge_index[1].contiguous()


def edge_score_forward(z, row, col, sigmoid=False, lanes=0):
    """v [E] of mp_edge_score_f32 (no autograd, no checks: see edge_score)."""
    nat = _lib.native()
    E = row.numel()
    v = torch.empty(E, dtype=torch.float32, device=z.device)
    if E:
        _count_call(nat, "mp_edge_score_f32", row.data_ptr(), col.data_ptr(), E, z.data_ptr(), z.stride(0), z.shape[0],
                    z.shape[1], int(bool(sigmoid)), int(lanes), v.data_ptr(), _lib.nbytes(v), _lib.stream_ptr(z.device))
    return v


def link_loss_side(z, row, col, positive, lanes=0):
    """(loss [], coef [E]) of mp_link_loss_f32: the mean of -log(p + EPS)
    (positive) or -log(1 - p + EPS) over the edges, p the sigmoid of the score,
    and coef[e] = d loss / d v_e (no autograd, no checks: see link_loss)."""
    nat = _lib.native()
    dev = z.device
    E = row.numel()
    coef = torch.empty(E, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    wsb = nat.mp_link_loss_workspace(E)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _count_call(nat, "mp_link_loss_f32", _lib.ptr(row if E else None), _lib.ptr(col if E else None), E, z.data_ptr(),
                z.stride(0), z.shape[0], z.shape[1], int(bool(positive)), int(lanes), _lib.ptr(coef if E else None),
                _lib.nbytes(coef), loss.data_ptr(), 4, ws.data_ptr(), wsb, _lib.stream_ptr(dev))
    return loss[0], coef


def link_pair_csr(row, col, n):
    """(rowptr, col, eid) int32 of mp_csr_build over the 2 E entries key = [row |
    col], other = [col | row]: node i's slots name, in edge order, the other end of
    every edge i is an end of (eid >= E: as its col).  Unscheduled, and the build's
    bad-index count is not read: no host read (the caller vouches for the range)."""
    nat = _lib.native()
    dev = row.device
    E2 = 2 * row.numel()
    key, other = torch.cat([row, col]), torch.cat([col, row])
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    c = torch.empty(max(E2, 1), dtype=torch.int32, device=dev)
    eid = torch.empty(max(E2, 1), dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = nat.mp_csr_build_workspace(E2, n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    nat.mp_csr_build(key.data_ptr(), other.data_ptr(), E2, n, n, rowptr.data_ptr(), c.data_ptr(), eid.data_ptr(),
                     bad.data_ptr(), ws.data_ptr(), wsb, _lib.stream_ptr(dev))
    return rowptr, c, eid, E2


def link_grad_rows(pair_csr, coef, z, out=None):
    """dz [N, C] (+= when out is given) = sum_{row_e = i} coef_e z[col_e] + sum_{col_e
    = i} coef_e z[row_e] over link_pair_csr's slots (mp_link_grad_rows_f32)."""
    nat = _lib.native()
    rowptr, c, eid, E2 = pair_csr
    N, C = z.shape
    init = out is not None
    if out is None:
        out = torch.empty((N, C), dtype=torch.float32, device=z.device)
    if N:
        _count_call(nat, "mp_link_grad_rows_f32", rowptr.data_ptr(), c.data_ptr(), eid.data_ptr(), N, E2,
                    _lib.ptr(coef if E2 else None), E2 // 2, _lib.ptr(z if E2 else None), z.stride(0), N, C, int(init),
                    out.data_ptr(), out.stride(0), _extent_bytes(out), _lib.stream_ptr(z.device))
    return out


def link_grad_engine(graph, coef, z, out=None):
    """The same gradient on the aggregation engine, for a cached edge list (graph =
    graph_for(edge_index, N, N)): two weighted row sums, over graph.dst then
    graph.src, the second into the first's output."""
    init = _lib.MP_FLAG_INIT_FROM_OUT if out is not None else 0
    if coef.numel() == 0:
        return out if out is not None else torch.zeros(z.shape, dtype=torch.float32, device=z.device)
    dst, src = graph.dst, graph.src
    out, _ = _aggregate(dst, "other", z, dst.to_csr_order(coef), "sum", init, None, out=out)
    _aggregate(src, "other", z, src.to_csr_order(coef), "sum", _lib.MP_FLAG_INIT_FROM_OUT, None, out=out)
    return out


def _link_grad(z, edge_index, row, col, coef, cached, out=None):
    from .graph import graph_for
    n = z.shape[0]
    if cached:
        return link_grad_engine(graph_for(edge_index, n, n), coef, z, out)
    return link_grad_rows(link_pair_csr(row, col, n), coef, z, out)


class _EdgeScore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, edge_index, row, col, sigmoid, cached):
        v = edge_score_forward(z, row, col, sigmoid)
        ctx.save_for_backward(z, edge_index, row, col, v)
        ctx.sigmoid, ctx.cached = sigmoid, cached
        return v

    @staticmethod
    def backward(ctx, g):
        z, edge_index, row, col, v = ctx.saved_tensors
        coef = g.to(torch.float32).contiguous()
        if ctx.sigmoid:
            coef = coef * (v * (1.0 - v))
        return _link_grad(z, edge_index, row, col, coef, ctx.cached), None, None, None, None, None


def edge_score(z, edge_index, sigmoid=False, cached=True):
    """v[e] = <z[row_e], z[col_e]> (or its sigmoid) for an int64 [2, E] edge list
    in any order, differentiable in z: InnerProductDecoder.forward without the two
    [E, C] gathers.  The backward sums coef_e z[other end] per node in edge order,
    deterministic and without float atomics: on the aggregation engine over the
    edge list's cached CSRs (cached=True: graph_for, one host read the first
    time the tensor is seen), or over an unscheduled CSR built on the spot with no
    host read (cached=False: edge lists that are new every step)."""
    z, row, col = _link_args(z, edge_index, "edge_score")
    return _EdgeScore.apply(z, edge_index, row, col, bool(sigmoid), bool(cached))


class _LinkLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, pos, prow, pcol, nrow, ncol):
        lp, cp = link_loss_side(z, prow, pcol, True)
        ln, cn = link_loss_side(z, nrow, ncol, False)
        ctx.save_for_backward(z, pos, prow, pcol, nrow, ncol, cp, cn)
        return lp + ln

    @staticmethod
    def backward(ctx, g):
        z, pos, prow, pcol, nrow, ncol, cp, cn = ctx.saved_tensors
        g = g.to(torch.float32)
        dz = _link_grad(z, pos, prow, pcol, cp * g, True)
        if nrow.numel():
            dz = _link_grad(z, None, nrow, ncol, cn * g, False, out=dz)
        return dz, None, None, None, None, None


def link_loss(z, pos_edge_index, neg_edge_index, neg_trusted=False):
    """GAE's reconstruction loss with the inner-product decoder, fused:
    mean(-log(sigmoid(v_pos) + 1e-15)) + mean(-log(1 - sigmoid(v_neg) + 1e-15)), one
    pass per side that also writes d loss / d v_e, each mean carried in fp64 in a
    fixed order.  The backward never forms the scores again: the positive edges go
    through the engine over pos_edge_index's cached CSRs, the negative ones --
    new every step -- through an unscheduled CSR (mp_link_grad_rows_f32), scaled by
    the incoming gradient on the device.  An empty side gives nan, as upstream's
    mean of nothing.  neg_trusted: the negatives come from negative_sample and need
    no range check (no host read)."""
    z, prow, pcol = _link_args(z, pos_edge_index, "link_loss")
    _, nrow, ncol = _link_args(z, neg_edge_index, "link_loss", trusted=neg_trusted)
    return _LinkLoss.apply(z, pos_edge_index, prow, pcol, nrow, ncol)


def _key_table(edge_index, n, upper=False, loops=False):
    """The cached KeyTable (graph.key_table_for) of the pairs a sampler over
    edge_index must not return.  upper: the undirected pairs i < j as j (j - 1) / 2
    + i; else row * n + col, with every (i, i) added when loops (the edge list
    GAE.recon_loss samples against: self loops removed, then one per node).  Built
    with a key sort and a dedupe, reading the table's size (and the loop count)
    once per edge_index tensor."""
    from .graph import KeyTable, key_table_for
    _lib.require_device(edge_index)
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("mi355_mp: edge_index must be int64 [2, E] (got %s %s)"
                         % (edge_index.dtype, tuple(edge_index.shape)))
    n = int(n)
    if n < 0 or n > 3037000499:
        raise ValueError("mi355_mp: num_nodes = %d is outside [0, 3037000499]" % n)
    check_row_index(edge_index, n, "negative_sampling")

    def build():
        row, col = edge_index[0], edge_index[1]
        n_edges = row.numel()
        if upper:
            keep = row != col
            lo, hi = torch.minimum(row, col)[keep], torch.maximum(row, col)[keep]
            key = ((hi * (hi - 1)) >> 1) + lo
        else:
            key = row * n + col
            if loops:
                n_edges += n - int((row == col).sum())
                ar = torch.arange(n, dtype=torch.int64, device=row.device)
                key = torch.cat([key, ar * n + ar])
        return KeyTable(torch.unique(key), n_edges, n, upper)
    return key_table_for(edge_index, ("keys", n, bool(upper), bool(loops)), build)


def _sample_seed(seed, device):
    return dropout_seed(device) if seed is None else int(seed) & _MASK64


def negative_sample(edge_index, num_nodes, num_neg_samples=None, force_undirected=False, seed=None, loops=False):
    """[2, n] int64 pairs that are not edges of edge_index, drawn uniformly WITH
    replacement (upstream's first round draws without; a pair can repeat here)
    by mp_neg_sample: draw s is the r-th key outside the cached sorted key table,
    r = mulhi64(mix(mix(seed) ^ s), #non-edges) -- no rejection loop, no retry,
    nothing read back.  n = min(num_neg_samples or E, N^2 - E), E the edge count
    (after the loop rewrite when loops: see _key_table); force_undirected draws n
    // 2 pairs i < j of the strict upper triangle that are in neither direction
    and returns them with their mirrors, [i | j ; j | i].  When no pair is
    missing the result is empty.  seed: None takes dropout_seed(device), so
    torch.cuda.manual_seed repeats the sequence."""
    nat = _lib.native()
    table = _key_table(edge_index, num_nodes, upper=force_undirected, loops=loops)
    dev = edge_index.device
    N, E = table.n_nodes, table.n_edges
    n = max(min(int(num_neg_samples or E), N * N - E), 0)
    if force_undirected:
        n //= 2
    total = N * (N - 1) // 2 if force_undirected else N * N
    if total - table.count <= 0:
        n = 0
    cols = 2 * n if force_undirected else n
    out = torch.empty((2, cols), dtype=torch.int64, device=dev)
    if n:
        _count_call(nat, "mp_neg_sample", _lib.ptr(table.keys if table.count else None), _lib.nbytes(table.keys),
                    table.n_keys.data_ptr(), N, _lib.MP_NEG_UPPER if force_undirected else _lib.MP_NEG_FULL,
                    _sample_seed(seed, dev), n, out[0].data_ptr(), out[1].data_ptr(), cols * 8, _lib.stream_ptr(dev))
    return out


def structured_negative_sample(edge_index, num_nodes, seed=None):
    """k [E] int64: for every edge (i, j) a node k with (i, k) not an edge, uniform
    over row i's missing columns (mp_neg_sample_rows; with replacement across
    edges, as upstream).  A node linked to every node has no such k: its edges get
    -1, where upstream's rejection loop would never end."""
    nat = _lib.native()
    table = _key_table(edge_index, num_nodes)
    dev = edge_index.device
    row = edge_index[0].contiguous()
    E = row.numel()
    out = torch.empty(E, dtype=torch.int64, device=dev)
    if E:
        _count_call(nat, "mp_neg_sample_rows", _lib.ptr(table.keys if table.count else None), _lib.nbytes(table.keys),
                    table.n_keys.data_ptr(), table.n_nodes, _sample_seed(seed, dev), row.data_ptr(), E, out.data_ptr(),
                    E * 8, _lib.stream_ptr(dev))
    return out
