"""Torch-tensor wrappers over the C ABI (include/cdseg.h).

Each function mirrors one reference call site (cited in include/cdseg.h) and is a thin
marshalling layer: PyTorch provides device memory and the stream, every computation runs in
the hand-written HIP kernels of libcdseg_hip.so.  No fallbacks: tensors must live on a GPU.
"""
import collections
import ctypes
import math
import os
import threading

import torch

from . import _lib
from ._lib import ACT_GELU, ACT_NONE, ACT_SWISH, BF16, F32, GemmArgs, check

__all__ = ["ACT_NONE", "ACT_GELU", "ACT_SWISH", "F32", "BF16"]

LP_DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}  # the 16-bit type of each build of the library


class _Dtypes:
    """torch dtype -> ABI dtype code.  A 16-bit tensor must be of the ACTIVE build's 16-bit type (`_lib.use`): the ABI
    code CDSEG_BF16 means "the build's 16-bit type", handing half bits to the bfloat16 build would compute garbage."""

    def __getitem__(self, dtype):
        if dtype == torch.float32:
            return F32
        if dtype == LP_DTYPES[_lib.active()]:
            return BF16
        raise _lib.CdsegError(f"{dtype} tensors do not belong to the active build of the library ({_lib.active()})")


_DT = _Dtypes()


def is_lp(dtype):
    return dtype in (torch.bfloat16, torch.float16)


_WS = {}
_GEMM_WS_BYTES = {}  # (m, N, gathered, fused LayerNorm) -> cdseg_gemm_ws_bytes


class _LazyLib:
    """Attribute access loads the library on first use (and raises loudly if it is missing)."""

    def __getattr__(self, name):
        return getattr(_lib.load(), name)


_LIB = _LazyLib()


class KernelTimer:
    """HIP-event timing of selected ops on the stream they are launched on (torch's current
    stream).  bench.py installs one over the timed region to get per-kernel durations live."""

    def __init__(self, names=("attention",)):
        self.names = set(names)
        self.events = []

    def begin(self, name):
        if name not in self.names:
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return (name, e0)

    def end(self, tok, work=0.0):
        if tok is None:
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.events.append((tok[0], tok[1], e1, work))

    def summary(self):
        """name -> dict(launches, ms, work) ; call after torch.cuda.synchronize()."""
        out = {}
        for name, e0, e1, work in self.events:
            d = out.setdefault(name, dict(launches=0, ms=0.0, work=0.0))
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["work"] += work
        return out


TIMER = None


def _loaded_libs():
    """Every build of the library this process has loaded (a process normally runs one precision, but the 16-bit type is
    a per-thread choice: profiling switches and summaries must not depend on which thread asks - ADVICE r3)."""
    libs = list(_lib._libs.values())
    return libs if libs else [_lib.load()]


def attention_prof_enable(on=True):
    """Event-time every attention / sparse-conv launch inside the library (works for the native Block executor too); applies
    to every loaded build."""
    for lib in _loaded_libs():
        check(lib.cdseg_prof_enable(1 if on else 0), "prof_enable")


def attention_prof_summary():
    """(total_ms, launches) since attention_prof_enable(True), summed over the loaded builds; call after torch.cuda.synchronize()."""
    return prof_summary(PROF_ATTENTION)


PROF_ATTENTION, PROF_CONV, PROF_CONV_DEEP = 0, 1, 2  # include/cdseg.h


# ------------------------------------------------------------------ launch record (include/cdseg.h: cdseg_route_*)
ROUTE_WORDS = 8
ROUTE_F_VEC_OK, ROUTE_F_GATHER, ROUTE_F_PARTIALS, ROUTE_F_KDIV, ROUTE_F_KSHIFT_LT6, ROUTE_F_CT_SHIFT = 1, 2, 4, 8, 16, 5


class Route(collections.namedtuple("Route", "kernel bm bn splits fix xmode flags aux")):
    """One recorded launch: `kernel` is the catalogue name; the flag bits as properties."""
    __slots__ = ()
    vec_ok = property(lambda r: bool(r.flags & ROUTE_F_VEC_OK))
    gather = property(lambda r: bool(r.flags & ROUTE_F_GATHER))
    partials = property(lambda r: bool(r.flags & ROUTE_F_PARTIALS))
    kdiv = property(lambda r: bool(r.flags & ROUTE_F_KDIV))
    kshift_lt6 = property(lambda r: bool(r.flags & ROUTE_F_KSHIFT_LT6))
    compute = property(lambda r: (r.flags >> ROUTE_F_CT_SHIFT) & 3)


def route_catalog(lib=None):
    """Names of every kernel id compiled into the (calling thread's active) build, in id order."""
    lib = lib or _lib.load()
    need = lib.cdseg_route_catalog(None, 0)
    buf = ctypes.create_string_buffer(need)
    assert lib.cdseg_route_catalog(buf, need) == need
    return buf.value.decode().split("\n")


def route_read(lib=None, capacity=64):
    """(launches recorded by this thread since the last clear, the newest `capacity` of them as Route tuples, oldest first)."""
    lib = lib or _lib.load()
    rec = (ctypes.c_int32 * (ROUTE_WORDS * max(capacity, 1)))(*([-1] * (ROUTE_WORDS * max(capacity, 1))))
    count = lib.cdseg_route_read(rec, capacity)
    names = route_catalog(lib)
    # the library writes min(count, its ring, capacity) records and nothing behind them: a kernel id is never negative, so the
    # rows written are the ones whose id no longer holds the -1 put there (no ring size is assumed on this side)
    rows = [list(rec[ROUTE_WORDS * i:ROUTE_WORDS * (i + 1)]) for i in range(min(count, capacity))]
    rows = [r for r in rows if r[0] >= 0]
    return count, [Route(names[r[0]], *r[1:]) for r in rows]


class record_routes:
    """`with ops.record_routes() as rr: ...` - afterwards rr.count / rr.routes hold what the calling thread's launches in the
    active build recorded inside the block (which kernel each host-side chooser picked).  Tests and diagnostics only."""

    def __enter__(self):
        self.lib = _lib.load()
        self.prev = self.lib.cdseg_route_enable(1)
        self.lib.cdseg_route_clear()
        self.count, self.routes = 0, []
        return self

    def __exit__(self, *exc):
        self.count, self.routes = route_read(self.lib)
        self.lib.cdseg_route_enable(self.prev)
        return False

    def kernels(self):
        return [r.kernel for r in self.routes]


def prof_summary(cls):
    """(total_ms, launches) of one profiled kernel class since attention_prof_enable(True), summed over the loaded builds;
    after a device sync."""
    tot_ms, tot_cnt = 0.0, 0
    for lib in _loaded_libs():
        ms, cnt = ctypes.c_double(0.0), ctypes.c_long(0)
        check(lib.cdseg_prof_summary_class(int(cls), ctypes.byref(ms), ctypes.byref(cnt)), "prof_summary_class")
        tot_ms += ms.value
        tot_cnt += cnt.value
    return tot_ms, tot_cnt


def set_timer(t):
    global TIMER
    TIMER = t


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _ThreadState(threading.local):
    """Per host thread: the bound stream, the GEMM argument-block cache and the Block I/O struct (inference_many
    issues each lane from its own thread; ctypes structs are filled in place, so they cannot be shared)."""

    def __init__(self):
        self.stream = None      # ctypes.c_void_p of the bound HIP stream
        self.stream_obj = None  # the torch stream object
        self.gemm_cache = {}
        self.f32x3 = False  # fp32 products of this thread's calls run as three half MFMAs on split operands (set_f32x3)
        self.block_io = None


_TLS = _ThreadState()


def bind_stream(stream=None):
    """Cache the HIP stream every op of THIS THREAD launches on (torch.cuda.current_stream() costs ~8 us per query,
    and an inference issues ~500 launches).  The engine binds the current torch stream once per inference call and
    re-binds when it switches to its side stream."""
    if stream is None:
        stream = torch.cuda.current_stream()
    _TLS.stream_obj = stream
    _TLS.stream = ctypes.c_void_p(stream.cuda_stream)
    return _TLS.stream


def unbind_stream():
    _TLS.stream = _TLS.stream_obj = None


def current_stream_id():
    """Identity of the bound stream (None when nothing is bound)."""
    st = _TLS.stream
    return st.value if st is not None else None


def record_event():
    ev = torch.cuda.Event()
    ev.record(_TLS.stream_obj if _TLS.stream_obj is not None else torch.cuda.current_stream())
    return ev


def wait_event(ev):
    (_TLS.stream_obj if _TLS.stream_obj is not None else torch.cuda.current_stream()).wait_event(ev)


def _stream():
    st = _TLS.stream
    return st if st is not None else ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.CdsegError("cdsegnet_amd ops run on the GPU only (HIP kernels); got a CPU tensor")


def dt(t):
    return _DT[t.dtype]


def workspace(nbytes, device):
    """Per-device scratch buffer (grown geometrically, never shrunk)."""
    key = (device.type, device.index, current_stream_id())  # one buffer per stream
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def _scratch(nbytes, device):
    """A fresh byte buffer of exactly nbytes from torch's allocator: the per-call workspaces of the training kernels, the packed
    weight images and the plan arenas, each sized by its cdseg_*_bytes / *_layout function (one place, so that a test can serve
    guarded views: tests/test_gpu_workspace_contract.py)."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------ serialization
def grid_max(grid):
    _need_gpu(grid)
    grid = grid.contiguous()
    out = torch.empty(1, dtype=torch.int64, device=grid.device)
    check(_lib.load().cdseg_grid_max(_ptr(grid), grid.element_size(), grid.numel(), _ptr(out), _stream()), "grid_max")
    return out


def offset2batch(offset, n):
    _need_gpu(offset)
    offset = offset.contiguous().to(torch.int64)
    out = torch.empty(n, dtype=torch.int32, device=offset.device)
    check(_lib.load().cdseg_offset2batch(_ptr(offset), offset.numel(), n, _ptr(out), _stream()), "offset2batch")
    return out


def encode(grid, batch, depth, order):
    """serialization/default.py:8-24.  grid (N,3) int32|int64; batch None|int32|int64 -> int64 codes."""
    _need_gpu(grid, batch)
    grid = grid.contiguous()
    n = grid.shape[0]
    code = torch.empty(n, dtype=torch.int64, device=grid.device)
    b = None if batch is None else batch.contiguous()
    oid = _lib.ORDER_IDS[order] if isinstance(order, str) else int(order)
    check(_lib.load().cdseg_encode(_ptr(grid), grid.element_size(), _ptr(b), 0 if b is None else b.element_size(), n,
                                   int(depth), oid, _ptr(code), _stream()), "encode")
    return code


def encode4(grid_i32, batch_i32, depth):
    _need_gpu(grid_i32, batch_i32)
    n = grid_i32.shape[0]
    code = torch.empty((4, n), dtype=torch.int64, device=grid_i32.device)
    check(_lib.load().cdseg_encode4(_ptr(grid_i32), _ptr(batch_i32), n, int(depth), _ptr(code), _stream()), "encode4")
    return code


def sort_pairs(keys, vals=None, end_bit=64):
    """Stable radix sort of non-negative int64 keys with int32 payload (iota if vals is None)."""
    _need_gpu(keys, vals)
    lib = _lib.load()
    keys = keys.contiguous()
    n = keys.numel()
    keys_out = torch.empty_like(keys)
    vals_out = torch.empty(n, dtype=torch.int32, device=keys.device)
    nbytes = lib.cdseg_sort_ws_bytes(n)
    ws = workspace(nbytes, keys.device)
    check(lib.cdseg_sort_pairs(_ptr(keys), _ptr(keys_out), _ptr(vals), _ptr(vals_out), n, int(end_bit), _ptr(ws),
                               ws.numel(), _stream()), "sort_pairs")
    return keys_out, vals_out


def sort_curves(code4, rows, end_bit):
    """Orders (rank -> row, int32) of the curve rows ``rows`` of code4 (4, n) with ONE radix sort (the curve slot rides in
    the key bits above end_bit): returns a (len(rows), n) int32 tensor, row k = argsort of code4[rows[k]]."""
    _need_gpu(code4)
    lib = _lib.load()
    n, count = code4.shape[1], len(rows)
    orders = torch.empty((count, n), dtype=torch.int32, device=code4.device)
    if n == 0 or count == 0:
        return orders
    ws = workspace(lib.cdseg_sort_curves_ws_bytes(n, count), code4.device)
    arr = (ctypes.c_int * count)(*[int(r) for r in rows])
    check(lib.cdseg_sort_curves(_ptr(code4), arr, count, n, int(end_bit), _ptr(orders), _ptr(ws), ws.numel(), _stream()),
          "sort_curves")
    return orders


def invert_perm(perm):
    _need_gpu(perm)
    inv = torch.empty_like(perm)
    check(_lib.load().cdseg_invert_perm(_ptr(perm), perm.numel(), _ptr(inv), _stream()), "invert_perm")
    return inv


def widen(x_i32):
    out = torch.empty(x_i32.shape, dtype=torch.int64, device=x_i32.device)
    check(_lib.load().cdseg_widen_i32(_ptr(x_i32), x_i32.numel(), _ptr(out), _stream()), "widen")
    return out


def gather_rows(src, idx):
    """dst[i] = src[idx[i]] (rows), idx int32, idx<0 -> zero row."""
    _need_gpu(src, idx)
    src = src.contiguous()
    row_bytes = src[0].numel() * src.element_size() if src.dim() > 1 else src.element_size()
    out = torch.empty((idx.numel(),) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    check(_lib.load().cdseg_gather_rows(_ptr(src), _ptr(idx), idx.numel(), row_bytes, _ptr(out), _stream()),
          "gather_rows")
    return out


def scatter_rows(src, idx, out):
    _need_gpu(src, idx, out)
    src = src.contiguous()
    row_bytes = src[0].numel() * src.element_size() if src.dim() > 1 else src.element_size()
    check(_lib.load().cdseg_scatter_rows(_ptr(src), _ptr(idx), idx.numel(), row_bytes, _ptr(out), _stream()),
          "scatter_rows")
    return out


def gather_i32(src, idx):
    out = torch.empty(idx.numel(), dtype=torch.int32, device=src.device)
    check(_lib.load().cdseg_gather_i32(_ptr(src), _ptr(idx), idx.numel(), _ptr(out), _stream()), "gather_i32")
    return out


def plan_gather_grid(grid, perm, zcode_sorted, depth):
    grid = grid.contiguous()
    n = grid.shape[0]
    g = torch.empty((n, 3), dtype=torch.int32, device=grid.device)
    b = torch.empty(n, dtype=torch.int32, device=grid.device)
    check(_lib.load().cdseg_plan_gather_grid(_ptr(grid), grid.element_size(), _ptr(perm), _ptr(zcode_sorted), n,
                                             int(depth), _ptr(g), _ptr(b), _stream()), "plan_gather_grid")
    return g, b


def pool_level(zcode_sorted, shift_bits, count_out=None):
    """Clusters of z-sorted points at one pooling level -> (cluster (n), seg_start (n+1, first count+1 valid),
    count (1,) int32 on device)."""
    lib = _lib.load()
    n = zcode_sorted.numel()
    dev = zcode_sorted.device
    cluster = torch.empty(n, dtype=torch.int32, device=dev)
    seg_start = torch.empty(n + 1, dtype=torch.int32, device=dev)
    count = count_out if count_out is not None else torch.empty(1, dtype=torch.int32, device=dev)
    ws = workspace(lib.cdseg_sort_ws_bytes(n), dev)
    check(lib.cdseg_pool_level(_ptr(zcode_sorted), n, int(shift_bits), _ptr(cluster), _ptr(seg_start), _ptr(count),
                               _ptr(ws), ws.numel(), _stream()), "pool_level")
    return cluster, seg_start, count


def pool_levels(zcode_sorted, shifts, last_idx):
    """All pooling levels at once -> (cluster (L,n), seg_start (L,n+1), meta) int32 on the device; meta is FLAT:
    L x (1+nb) ints [pooled count, cluster of each batch element's last point] then one int = duplicate-voxel count."""
    lib = _lib.load()
    n, L, nb = zcode_sorted.numel(), len(shifts), last_idx.numel()
    dev = zcode_sorted.device
    cluster = torch.empty((L, n), dtype=torch.int32, device=dev)
    seg = torch.empty((L, n + 1), dtype=torch.int32, device=dev)
    meta = torch.empty(L * (1 + nb) + 1, dtype=torch.int32, device=dev)
    ws = workspace(lib.cdseg_pool_levels_ws_bytes(n, L), dev)
    sh = (ctypes.c_int * L)(*[int(v) for v in shifts])
    check(lib.cdseg_pool_levels(_ptr(zcode_sorted), n, sh, L, _ptr(last_idx), nb, _ptr(cluster), _ptr(seg), _ptr(meta),
                                _ptr(ws), ws.numel(), _stream()), "pool_levels")
    return cluster, seg, meta


def link_derive(cl0a, seg0a, ma, cl0b, seg0b, mb):
    dev = cl0a.device
    cluster = torch.empty(int(ma), dtype=torch.int32, device=dev)
    seg = torch.empty(int(mb) + 1, dtype=torch.int32, device=dev)
    check(_lib.load().cdseg_link_derive(_ptr(cl0a), _ptr(seg0a), int(ma), _ptr(cl0b), _ptr(seg0b), int(mb),
                                         _ptr(cluster), _ptr(seg), _stream()), "link_derive")
    return cluster, seg


def coarse_orders(clusters, orders, sizes):
    """Curve orders of all pooled levels from the level-0 orders (no sort).  clusters: per level (n0) int32 cluster
    ids of the level-0 points; orders: per curve (n0) int32 rank -> level-0 point; sizes: per level m_l.
    Returns [[order of level l on curve c for c] for l] as views of one int32 buffer."""
    lib = _lib.load()
    n0 = clusters[0].numel()
    nl, nc = len(clusters), len(orders)
    dev = clusters[0].device
    out = torch.empty(nc * int(sum(sizes)), dtype=torch.int32, device=dev)
    ws = workspace(lib.cdseg_coarse_orders_ws_bytes(n0, nl, nc), dev)
    cp = (ctypes.c_void_p * nl)(*[t.data_ptr() for t in clusters])
    op = (ctypes.c_void_p * nc)(*[t.data_ptr() for t in orders])
    check(lib.cdseg_coarse_orders(cp, nl, op, nc, n0, _ptr(out), _ptr(ws), ws.numel(), _stream()), "coarse_orders")
    parts = out.split([int(m) for m in sizes for _ in range(nc)])
    return [list(parts[i * nc:(i + 1) * nc]) for i in range(nl)]


def pool_gather(seg_start, m, n_fine, pooling_depth, grid_f, batch_f, code4_f):
    dev = grid_f.device
    grid_c = torch.empty((m, 3), dtype=torch.int32, device=dev)
    batch_c = torch.empty(m, dtype=torch.int32, device=dev)
    code_c = torch.empty((4, m), dtype=torch.int64, device=dev)
    check(_lib.load().cdseg_pool_gather(_ptr(seg_start), m, n_fine, int(pooling_depth), _ptr(grid_f), _ptr(batch_f),
                                        _ptr(code4_f), _ptr(grid_c), _ptr(batch_c), _ptr(code_c), _stream()),
          "pool_gather")
    return grid_c, batch_c, code_c


def nbr_table(zcode_sorted, grid_i32, batch_i32, depth, ksize, kmajor=False):
    n = grid_i32.shape[0]
    kv = ksize ** 3
    shape = (kv, n) if kmajor else (n, kv)
    nbr = torch.empty(shape, dtype=torch.int32, device=grid_i32.device)
    check(_lib.load().cdseg_nbr_table(_ptr(zcode_sorted), _ptr(grid_i32), _ptr(batch_i32), n, int(depth), int(ksize),
                                      1 if kmajor else 0, _ptr(nbr), _stream()), "nbr_table")
    return nbr


def nbr_table_from_parent(zcode_sorted, grid_i32, cluster, parent_nbr3, seg_start, m, depth, ksize, kmajor=False):
    """Kernel map of a level from its parent level's (27, m) offset-major 3x3x3 map (pooling depth 1)."""
    n = zcode_sorted.numel()
    kv = ksize ** 3
    nbr = torch.empty((kv, n) if kmajor else (n, kv), dtype=torch.int32, device=zcode_sorted.device)
    check(_lib.load().cdseg_nbr_table_from_parent(_ptr(zcode_sorted), _ptr(grid_i32), _ptr(cluster), _ptr(parent_nbr3),
                                                   _ptr(seg_start), n, int(m), int(depth), int(ksize),
                                                   1 if kmajor else 0, _ptr(nbr), _stream()), "nbr_table_from_parent")
    return nbr


def nbr_table_from_info(grid_i32, cluster, parent_nbr3, child_info_words, m, depth, ksize, kmajor=False):
    """The same from the parents' child_info words (first child row << 8 | octant occupancy) instead of the children runs:
    two dependent reads per (point, offset)."""
    n = grid_i32.shape[0]
    kv = ksize ** 3
    nbr = torch.empty((kv, n) if kmajor else (n, kv), dtype=torch.int32, device=grid_i32.device)
    check(_lib.load().cdseg_nbr_table_from_info(_ptr(grid_i32), _ptr(cluster), _ptr(parent_nbr3), _ptr(child_info_words), n,
                                                 int(m), int(depth), int(ksize), 1 if kmajor else 0, _ptr(nbr), _stream()),
          "nbr_table_from_info")
    return nbr


def pad_plan(order, offs, offs_pad, patch, n_pad):
    dev = offs.device
    gidx = torch.empty(n_pad, dtype=torch.int32, device=dev)
    widx = torch.empty(n_pad, dtype=torch.int32, device=dev)
    check(_lib.load().cdseg_pad_plan(_ptr(order), _ptr(offs), _ptr(offs_pad), offs.numel() - 1, int(patch), n_pad,
                                     _ptr(gidx), _ptr(widx), _stream()), "pad_plan")
    return gidx, widx


SLOTS_SELECT_MAX = 64  # include/cdseg.h CDSEG_SLOTS_SELECT_MAX


def slots_select(sources, offs_pad, choice, n_pad):
    """Slot plan of a collated batch whose elements read different curves: out[s] = sources[choice[b]][s] for every padded
    slot s of batch element b.  sources: up to four (gidx, widx) pairs of n_pad int32 each (the slot plans of one level and
    patch key), None where no element chooses it; offs_pad (nb + 1) int32 on the device; choice: nb host ints.  The choices
    ride in the launch arguments: no host-to-device copy.  -> (gidx, widx)."""
    choice = [int(c) for c in choice]
    _need_gpu(offs_pad)
    if offs_pad.dtype != torch.int32 or not offs_pad.is_contiguous():
        raise _lib.CdsegError("slots_select: offs_pad is a contiguous int32 tensor")
    if len(choice) != offs_pad.numel() - 1 or any(c < 0 or c > 255 for c in choice):
        raise _lib.CdsegError("slots_select: one choice in 0..255 per batch element")
    k = len(sources)
    dev = offs_pad.device
    gsrc = (ctypes.c_void_p * max(1, k))(*[None if s is None else s[0].data_ptr() for s in sources])
    wsrc = (ctypes.c_void_p * max(1, k))(*[None if s is None else s[1].data_ptr() for s in sources])
    for s in sources:
        if s is not None and (s[0].numel() != n_pad or s[1].numel() != n_pad or s[0].dtype != torch.int32 or
                              s[1].dtype != torch.int32 or not s[0].is_contiguous() or not s[1].is_contiguous()):
            raise _lib.CdsegError("slots_select: every source is a pair of contiguous int32 tensors of n_pad elements")
    gidx = torch.empty(n_pad, dtype=torch.int32, device=dev)
    widx = torch.empty(n_pad, dtype=torch.int32, device=dev)
    check(_lib.load().cdseg_slots_select(gsrc, wsrc, k, _ptr(offs_pad), len(choice), bytes(choice), int(n_pad), _ptr(gidx),
                                         _ptr(widx), _stream()), "slots_select")
    return gidx, widx


# ------------------------------------------------------------------ native plan builder (csrc/plan.hip)
class NativePlanCall:
    """One forward's plan through cdseg_plan_begin / cdseg_plan_finish: owns the two arenas of each call and hands out views.
    `spec` is a filled _lib.PlanSpec (static per model and serialization depth)."""

    def __init__(self, spec, grid, offset_dev, n, nb, depth, end_bit, gmax_pin, meta_pin):
        lib = _lib.load()
        self.lib, self.spec, self.n, self.nb, self.depth = lib, spec, int(n), int(nb), int(depth)
        self.sp = ctypes.byref(spec)
        off = (ctypes.c_long * 13)()
        tot = (ctypes.c_long * 3)()
        check(lib.cdseg_plan_begin_layout(self.sp, self.n, self.nb, off, tot), "plan_begin_layout")
        dev = grid.device
        self.b32 = _scratch(4 * tot[0], dev).view(torch.int32)
        self.b64 = _scratch(8 * tot[1], dev).view(torch.int64)
        self.ws = workspace(tot[2], dev)
        self.boff = list(off)
        io = self.bio = _lib.PlanBeginIO()
        io.grid, io.grid_elem_bytes, io.offset = grid.data_ptr(), grid.element_size(), offset_dev.data_ptr()
        io.nb, io.n, io.depth, io.end_bit = self.nb, self.n, self.depth, int(end_bit)
        io.i32, io.i64, io.ws, io.ws_bytes = self.b32.data_ptr(), self.b64.data_ptr(), self.ws.data_ptr(), self.ws.numel()
        io.gmax_host = None if gmax_pin is None else gmax_pin.data_ptr()
        io.meta_host = meta_pin.data_ptr()
        self._keep = (grid, offset_dev)

    def begin(self, phase):
        check(self.lib.cdseg_plan_begin(self.sp, ctypes.byref(self.bio), int(phase), _stream()), "plan_begin")

    def begin_views(self):
        """perm0 (n), grid0 (n, 3), bat0 (n), code0 (4, n), cluster (nlev, n), seg_start (nlev, n + 1), orders0 (ncurve, n)."""
        o, n, b32, b64, L, nc = self.boff, self.n, self.b32, self.b64, self.spec.nlev, self.spec.ncurve
        return (b32[o[1]:o[1] + n], b32[o[2]:o[2] + 3 * n].view(n, 3), b32[o[3]:o[3] + n],
                b64[o[12]:o[12] + 4 * n].view(4, n), b32[o[5]:o[5] + L * n].view(L, n),
                b32[o[6]:o[6] + L * (n + 1)].view(L, n + 1), b32[o[8]:o[8] + nc * n].view(nc, n) if nc else None)

    def finish(self, m, offs_rows, pads_pin):
        """m: pooled sizes; offs_rows: (nlev + 1) lists of nb + 1 batch offsets; pads_pin(count) -> pinned int32 tensor with
        at least `count` elements (called once).  Returns (off, info): the layout lists of include/cdseg.h."""
        lib, spec, L, npad = self.lib, self.spec, self.spec.nlev, self.spec.npad
        mh = (ctypes.c_long * L)(*m)
        flat = [v for r in offs_rows for v in r]
        oh = (ctypes.c_int * len(flat))(*flat)
        n_off = 3 * L + 2 * spec.nlink + 2 * (L + 1) + 1 + 3 * (L + 1) * npad + 2
        n_info = 5 + 5 * (L + 1) * npad
        off = (ctypes.c_long * n_off)()
        info = (ctypes.c_long * n_info)()
        check(lib.cdseg_plan_finish_layout(self.sp, self.n, self.nb, mh, oh, off, info), "plan_finish_layout")
        dev = self.b32.device
        self.f32 = _scratch(4 * info[0], dev).view(torch.int32)
        self.f64 = _scratch(8 * max(1, info[1]), dev).view(torch.int64)
        if info[2] > self.ws.numel():
            self.ws = workspace(info[2], dev)
        pin = pads_pin(info[3])
        o, n, b32, b64 = self.boff, self.n, self.b32, self.b64
        io = _lib.PlanFinishIO()
        io.n, io.nb, io.depth, io.m_host, io.offs_host = self.n, self.nb, self.depth, mh, oh
        io.grid0 = b32.data_ptr() + 4 * o[2]
        io.bat0 = b32.data_ptr() + 4 * o[3]
        io.code0 = b64.data_ptr() + 8 * o[12]
        io.cluster = b32.data_ptr() + 4 * o[5]
        io.seg = b32.data_ptr() + 4 * o[6]
        io.orders0 = b32.data_ptr() + 4 * o[8]
        io.i32, io.i64, io.ws, io.ws_bytes = self.f32.data_ptr(), self.f64.data_ptr(), self.ws.data_ptr(), self.ws.numel()
        io.pads_host = pin.data_ptr()
        check(lib.cdseg_plan_finish(self.sp, ctypes.byref(io), _stream()), "plan_finish")
        return list(off), list(info)


# ------------------------------------------------------------------ float ops
PAD_BATCH_MAX = 48


def pad_plan_batch(items, nb):
    """items: list of (order or None, offs, offs_pad, patch, n_pad) -> list of (gidx, widx), one launch."""
    lib = _lib.load()
    res = []
    for s0 in range(0, len(items), PAD_BATCH_MAX):
        chunk = items[s0:s0 + PAD_BATCH_MAX]
        k = len(chunk)
        total = sum(int(it[4]) for it in chunk)
        dev = chunk[0][1].device
        gidx = torch.empty(total, dtype=torch.int32, device=dev)
        widx = torch.empty(total, dtype=torch.int32, device=dev)
        orders = (ctypes.c_void_p * k)(*[None if it[0] is None else it[0].data_ptr() for it in chunk])
        offs = (ctypes.c_void_p * k)(*[it[1].data_ptr() for it in chunk])
        offs_pad = (ctypes.c_void_p * k)(*[it[2].data_ptr() for it in chunk])
        patch = (ctypes.c_int * k)(*[int(it[3]) for it in chunk])
        npad = (ctypes.c_long * k)(*[int(it[4]) for it in chunk])
        check(lib.cdseg_pad_plan_batch(k, orders, offs, offs_pad, patch, npad, int(nb), _ptr(gidx), _ptr(widx), _stream()),
              "pad_plan_batch")
        sizes = [int(it[4]) for it in chunk]
        res.extend(zip(gidx.split(sizes), widx.split(sizes)))  # (one call per buffer: 2 k Python slices cost ~1.5 us each)
    return res


F32X3 = 2  # include/cdseg.h CDSEG_F32X3: fp32 in memory, split-half arithmetic on the matrix pipe


def set_f32x3(on):
    """This thread's fp32 `gemm` / `attention` calls compute in the split-half "fp32 x3" form (csrc/gemm.hip) from now on;
    returns the previous setting.  The engine of precision "fp32x3" brackets its forwards with it."""
    prev, _TLS.f32x3 = _TLS.f32x3, bool(on)
    return prev


def gemm(A, W, out, *, bias=None, scale=None, shift=None, act=ACT_NONE, res=None, add_src=None, add_idx=None,
         nbr=None, out_idx=None, out2=None, out2_pre_add=False, M=None, kvol=1, colbias=None, ln_pre=None,
         nbr_kmajor=False,
         ln_post=None, ln_out=None, ln_eps=1e-5, cache=True):
    """out = epilogue(A @ W^T) (or the gathered-A sparse-conv form when nbr is given).
    A (M,K) [or the gather source], W (N, kvol*K), both of the compute dtype.
    cache=False: W is a temporary (a transposed / mirrored copy made for this call, as the training backward does): the
    argument block is built on the spot and nothing keeps W alive afterwards."""
    if not A.is_cuda:
        _need_gpu(A, W, out)
    # the weight-side half of the argument block is static per layer: cache it keyed by the weight tensor
    x3 = _TLS.f32x3 and W.dtype == torch.float32
    key = (W.data_ptr(), _dp(bias), _dp(scale), _dp(shift), int(kvol), int(act), x3)
    cache_d = _TLS.gemm_cache
    ent = cache_d.get(key) if cache else None
    if ent is None:
        for t in (bias, scale, shift):
            if t is not None and t.dtype != torch.float32:
                raise _lib.CdsegError("gemm epilogue vectors are float32")
        a = GemmArgs()
        a.W, a.bias, a.scale, a.shift = key[0], key[1], key[2], key[3]
        a.N = W.shape[0]
        a.kvol = int(kvol)
        a.K = W.shape[1] // a.kvol
        a.compute_dtype = F32X3 if x3 else dt(W)
        a.act = int(act)
        ent = (a, ctypes.byref(a), W)  # keep W alive with the cache entry
        if cache:
            if len(cache_d) > 4096:
                cache_d.clear()
            cache_d[key] = ent
    a = ent[0]
    if (res is not None and res.dtype != torch.float32) or (add_src is not None and add_src.dtype != torch.float32):
        raise _lib.CdsegError("gemm residuals are float32")
    a.A = A.data_ptr()
    a.res, a.add_src, a.add_idx, a.nbr, a.out_idx = _dp(res), _dp(add_src), _dp(add_idx), _dp(nbr), _dp(out_idx)
    a.out, a.out2 = out.data_ptr(), _dp(out2)
    m = int(M if M is not None else (nbr.shape[1 if nbr_kmajor else 0] if nbr is not None else A.shape[0]))
    a.nbr_kmajor = 1 if nbr_kmajor else 0
    a.M = m
    a.lda = A.stride(0)
    a.ldo = out.stride(0)
    a.ldo2 = out2.stride(0) if out2 is not None else 0
    a.ldres = res.stride(0) if res is not None else 0
    a.ldadd = add_src.stride(0) if add_src is not None else 0
    a.a_dtype = _DT[A.dtype]
    a.out_dtype = _DT[out.dtype]
    a.out2_dtype = _DT[out2.dtype] if out2 is not None else 0
    a.out2_pre_add = 1 if out2_pre_add else 0
    a.colbias = _dp(colbias)
    if ln_pre is not None:
        a.ln_pre_g, a.ln_pre_b = ln_pre[0].data_ptr(), ln_pre[1].data_ptr()
    else:
        a.ln_pre_g = a.ln_pre_b = None
    if ln_post is not None:
        a.ln_post_g, a.ln_post_b = ln_post[0].data_ptr(), ln_post[1].data_ptr()
        a.ln_out, a.ldln, a.ln_out_dtype = ln_out.data_ptr(), ln_out.stride(0), _DT[ln_out.dtype]
    else:
        a.ln_post_g = a.ln_post_b = a.ln_out = None
    a.ln_eps = float(ln_eps)
    # cdseg_gemm_ws_bytes (the rule lives beside the launch plan it feeds, csrc/workspace.h), one lookup per repeated shape
    wkey = (m, a.N, nbr is not None, ln_pre is not None or ln_post is not None)
    want = _GEMM_WS_BYTES.get(wkey)
    if want is None:
        if len(_GEMM_WS_BYTES) > 4096:
            _GEMM_WS_BYTES.clear()
        want = _GEMM_WS_BYTES[wkey] = int(_lib.load().cdseg_gemm_ws_bytes(*wkey))
    if want:
        ws = workspace(want, out.device)
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    else:
        a.ws, a.ws_bytes = None, 0
    tok = TIMER.begin("conv" if nbr is not None else "gemm") if TIMER is not None else None
    check(_lib.load().cdseg_gemm(ent[1], _stream()), "gemm")
    if tok is not None:
        TIMER.end(tok, 2.0 * a.M * a.N * a.K * a.kvol)
    return out


FUSED_MLP_CHANNELS = (32, 64, 128)


def mlp_fused_ok(h, hidden):
    """The fused MLP kernel covers bf16 with C = 32 / 64 / 128 and the standard 4x hidden width."""
    c = h.shape[1]
    return (is_lp(h.dtype) and c in FUSED_MLP_CHANNELS and hidden == 4 * c and
            c <= 128)


def mlp_fused(h, w1, b1, w2, b2, x, xc=None):
    """x += fc2(GELU(fc1(h))), xc = bf16(x); the hidden activation never leaves the CU."""
    _need_gpu(h, x)
    check(_lib.load().cdseg_mlp_fused(_ptr(h), h.stride(0), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(x), x.stride(0),
                                       _ptr(xc), xc.stride(0) if xc is not None else 0, h.shape[0], h.shape[1], _DT[h.dtype],
                                       _stream()), "mlp_fused")
    return x


def cpe_head_fused_ok(y):
    """cpe linear + LN + residual + LN1 + qkv in one launch: bf16, C = 32 / 64."""
    return is_lp(y.dtype) and y.shape[1] in (32, 64)


def cpe_head_fused(y, wl, bl, lnp, x, colbias, ln1, wqkv, bqkv, qkv, eps=1e-5, qkv_flags=0):
    """x += LN_cpe(y Wl^T + bl) [+ colbias]; h = LN1(x); qkv = h Wqkv^T + bqkv.  qkv_flags: ATTN_V_BF16 = v third as bfloat16."""
    _need_gpu(y, x)
    check(_lib.load().cdseg_cpe_head_fused(_ptr(y), y.stride(0), _ptr(wl), _ptr(bl), _ptr(lnp[0]), _ptr(lnp[1]), _ptr(x),
                                            x.stride(0), _ptr(colbias), _ptr(ln1[0]), _ptr(ln1[1]), float(eps), _ptr(wqkv),
                                            _ptr(bqkv), _ptr(qkv), qkv.stride(0), y.shape[0], y.shape[1], _DT[y.dtype],
                                            int(qkv_flags), _stream()), "cpe_head_fused")
    return qkv


def attn_tail_fused_ok(o, hidden):
    """proj + LayerNorm + MLP in one launch: bf16, C = 32 / 64."""
    c = o.shape[1]
    return is_lp(o.dtype) and c in (32, 64) and hidden == 4 * c


def attn_tail_fused(o, wp, bp, ln_g, ln_b, w1, b1, w2, b2, x, xc=None, eps=1e-5):
    """x += proj(o); h = LN(x); x += fc2(GELU(fc1(h))); xc = bf16(x) - the Block's tail after attention."""
    _need_gpu(o, x)
    check(_lib.load().cdseg_attn_tail_fused(_ptr(o), o.stride(0), _ptr(wp), _ptr(bp), _ptr(ln_g), _ptr(ln_b), float(eps),
                                             _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(x), x.stride(0), _ptr(xc),
                                             xc.stride(0) if xc is not None else 0, o.shape[0], o.shape[1], _DT[o.dtype],
                                             _stream()), "attn_tail_fused")
    return x


# include/cdseg.h CDSEG_DEEP512_MIN_ROWS: below, a C = 512 Block keeps the separate GEMM launches.  Experimental builds of the
# library read the CDSEG_DEEP512_MIN_ROWS environment knob (csrc/runtime.hip); the binding path follows the same variable so
# that the two executors never disagree under an A/B run
DEEP512_MIN_ROWS = int(os.environ.get("CDSEG_DEEP512_MIN_ROWS", 2560))
# csrc/deep.hip DEEP512_ROWS64_MIN: from this many rows a C = 512 head / tail launch runs 64-row tiles (8 waves x 64 channels)
# instead of 32-row ones; the results are bit-identical, the constant is here for the tests and tools that compare the two
DEEP512_ROWS64_MIN = 256 * 32 + 1
DEEP_CHANNELS = (128, 256, 512)  # deep-stage head / tail kernels (csrc/deep.hip): weights streamed L2 -> registers


def block_rr_ok(channels, dtype):
    """Fused Block head / tail kernels on weight images: C = 32 / 64 (csrc/blockrr.hip: weights resident in LDS,
    activations in registers) and C = 128 / 256 / 512 (csrc/deep.hip: activations resident in LDS, weights streamed), 16-bit."""
    return is_lp(dtype) and (channels in (32, 64) or channels in DEEP_CHANNELS)


def block_rr_head_on(channels=32):
    """Deep stages: on.  The register-resident HEAD of the wide stages is off by default: the 64-row-tile fused head already streams at ~4.3 TB/s and measured
    5-10 % faster (tools/bench_block.py); the register-resident TAIL is 1.4-1.65x faster than its predecessor."""
    return channels in DEEP_CHANNELS


def block_rr_pack(channels, wl, wqkv, wp, w1, w2):
    """Fragment images of a Block's head (cpe linear, qkv) and tail (proj, fc1, fc2) weights -> (head_img, tail_img).
    wl = wqkv = None: the tail image alone (head_img None) - the cross block's tail has the Block's shape, its head not."""
    _need_gpu(wl, wqkv, wp, w1, w2)
    lib = _lib.load()
    dev = wp.device
    head = _scratch(lib.cdseg_block_rr_img_bytes(channels, 0), dev) if wl is not None else None
    tail = _scratch(lib.cdseg_block_rr_img_bytes(channels, 1), dev)
    check(lib.cdseg_block_rr_pack(int(channels), _ptr(wl), _ptr(wqkv), _ptr(head), _ptr(wp), _ptr(w1), _ptr(w2), _ptr(tail),
                                  _stream()), "block_rr_pack")
    return head, tail


def cpe_head_rr(y, head_img, bl, lnp, x, colbias, ln1, bqkv, qkv, eps=1e-5, qkv_flags=0):
    check(_lib.load().cdseg_cpe_head_rr(_ptr(y), y.stride(0), _ptr(head_img), _ptr(bl), _ptr(lnp[0]), _ptr(lnp[1]), _ptr(x),
                                        x.stride(0), _ptr(colbias), _ptr(ln1[0]), _ptr(ln1[1]), float(eps), _ptr(bqkv),
                                        _ptr(qkv), qkv.stride(0), y.shape[0], y.shape[1], int(qkv_flags), _stream()),
          "cpe_head_rr")
    return qkv


def cpe_head_rr2(y, head_img, bl, lnp, x, x_out, colbias, ln1, bqkv, qkv, eps=1e-5, qkv_flags=0):
    """Deep stages: `cpe_head_rr` with the residual rows read from x and written to x_out (distinct buffers let few-row launches
    split a tile over three workgroups, csrc/deep.hip)."""
    check(_lib.load().cdseg_cpe_head_rr2(_ptr(y), y.stride(0), _ptr(head_img), _ptr(bl), _ptr(lnp[0]), _ptr(lnp[1]), _ptr(x),
                                         x.stride(0), _ptr(x_out), x_out.stride(0), _ptr(colbias), _ptr(ln1[0]), _ptr(ln1[1]),
                                         float(eps), _ptr(bqkv), _ptr(qkv), qkv.stride(0), y.shape[0], y.shape[1],
                                         int(qkv_flags), _stream()), "cpe_head_rr2")
    return qkv


def attn_tail_rr2(o, tail_img, bp, ln_g, ln_b, b1, b2, x_in, x, xc=None, ws=None, eps=1e-5):
    """Deep stages: `attn_tail_rr` with the residual read from x_in, the result written to x; ws: fp32 / byte workspace that
    allows the few-row hidden-chunk split (>= 4 * n * C * 4 bytes for four workgroups per tile)."""
    check(_lib.load().cdseg_attn_tail_rr2(_ptr(o), o.stride(0), _ptr(tail_img), _ptr(bp), _ptr(ln_g), _ptr(ln_b), float(eps),
                                          _ptr(b1), _ptr(b2), _ptr(x_in), x_in.stride(0), _ptr(x), x.stride(0), _ptr(xc),
                                          xc.stride(0) if xc is not None else 0, o.shape[0], o.shape[1], _ptr(ws),
                                          0 if ws is None else ws.numel() * ws.element_size(), _stream()), "attn_tail_rr2")
    return x


def attn_tail_rr(o, tail_img, bp, ln_g, ln_b, b1, b2, x, xc=None, eps=1e-5):
    check(_lib.load().cdseg_attn_tail_rr(_ptr(o), o.stride(0), _ptr(tail_img), _ptr(bp), _ptr(ln_g), _ptr(ln_b), float(eps),
                                         _ptr(b1), _ptr(b2), _ptr(x), x.stride(0), _ptr(xc),
                                         xc.stride(0) if xc is not None else 0, o.shape[0], o.shape[1], _stream()),
          "attn_tail_rr")
    return x


def attn_tail_rr_ex(o, tail_img, bp, ln_g, ln_b, b1, b2, x, xc=None, eps=1e-5, flags=0, logits=None, head_w=None,
                    head_b=None, out_idx=None, num_classes=None, ld_logits=None):
    """`attn_tail_rr` with a say in what it writes (include/cdseg.h: cdseg_attn_tail_rr_ex).  flags: BLOCK_X_DEAD - x is read
    and left as it is, xc alone is stored.  logits (rows, classes) fp32 with head_w (classes, C) / head_b fp32 and out_idx (n)
    int32: neither x nor xc is written, the head's logits are (C = 64, classes % 4 == 0, classes <= 20).  num_classes /
    ld_logits default to head_w's rows / the logits' row stride."""
    if logits is not None:
        num_classes = head_w.shape[0] if num_classes is None else num_classes
        ld_logits = logits.stride(0) if ld_logits is None else ld_logits
    check(_lib.load().cdseg_attn_tail_rr_ex(_ptr(o), o.stride(0), _ptr(tail_img), _ptr(bp), _ptr(ln_g), _ptr(ln_b), float(eps),
                                            _ptr(b1), _ptr(b2), _ptr(x), x.stride(0), _ptr(xc),
                                            xc.stride(0) if xc is not None else 0, o.shape[0], o.shape[1], int(flags),
                                            _ptr(logits), int(ld_logits or 0), _ptr(head_w), _ptr(head_b), _ptr(out_idx),
                                            int(num_classes or 0), _stream()), "attn_tail_rr_ex")
    return x


def _dp(t):
    return None if t is None else t.data_ptr()


def make_block_desc(dtype, channels, heads, hidden, attn_scale, ln_eps, tensors, attn_flags=0, x3=False):
    """Describe one Block's weights once (tensors: dict field -> tensor); returns an object to pass to
    block_forward.  The tensors are kept alive by the returned handle.  attn_flags: ATTN_Q_PRESCALED when the q rows of
    qkv_w / qkv_b (and the images packed from them) carry attn_scale * log2(e)."""
    d = _lib.BlockDesc()
    d.dtype, d.channels, d.heads, d.hidden = (F32X3 if (x3 and dtype == torch.float32) else _DT[dtype]), int(channels), int(heads), int(hidden)
    d.attn_scale, d.ln_eps = float(attn_scale), float(ln_eps)
    d.attn_flags = int(attn_flags)
    for k, t in tensors.items():
        setattr(d, k, t.data_ptr())
    return (d, ctypes.byref(d), dict(tensors))


def block_scratch_bytes(desc, n):
    return _lib.load().cdseg_block_scratch_bytes(desc[1], int(n))


def count_saturated(x, counter):
    """Diagnostic of the IEEE-half build: counter (1-element int64 device tensor) += elements of the 16-bit matrix x that
    sit at +-65504, the clamp value of that build's float -> half conversions."""
    _need_gpu(x, counter)
    check(_lib.load().cdseg_count_saturated(_ptr(x), x.shape[0], x.shape[1], x.stride(0), _ptr(counter), _stream()),
          "count_saturated")


def split16(x, lo_scale=2048.0):
    """fp32 (rows, cols) -> (hi, lo) in the active build's 16-bit type: hi = T(x), lo = T((x - hi) * lo_scale)."""
    _need_gpu(x)
    T = LP_DTYPES[_lib.active()]
    hi = torch.empty(x.shape, dtype=T, device=x.device)
    lo = torch.empty(x.shape, dtype=T, device=x.device)
    check(_lib.load().cdseg_split16(_ptr(x), x.stride(0), x.shape[0], x.shape[1], _ptr(hi), _ptr(lo), hi.stride(0),
                                    float(lo_scale), _stream()), "split16")
    return hi, lo


def block_forward(desc, n, x, xc_in, xc_out, tbias, nbr, gidx, widx, patch_start, num_patches, max_len, scratch,
                  sat_counter=None, flags=0, logits=None, head_w=None, head_b=None, out_idx=None):
    """One PTv3 Block on the native executor (all launches issued by the library, one host call).  sat_counter: 1-element
    int64 device tensor that collects the Block's clamped half values (diagnostic, see count_saturated).
    flags: BLOCK_X_DEAD - the caller reads x no more, its contents are unspecified on return (the wide stages' tail then stores
    xc_out alone).  logits (rows, classes) fp32 with head_w (classes, C) / head_b fp32 and out_idx (n) int32: the model's last
    Block writes the head's logits instead of x and xc_out.  Returns False - nothing launched - when the library cannot
    (CDSEG_ERR_UNSUPPORTED: the caller runs the Block without them, then the head), True otherwise."""
    if _TLS.block_io is None:
        io = _lib.BlockIO()
        _TLS.block_io = (io, ctypes.byref(io))
    io, ref = _TLS.block_io
    io.n = int(n)
    io.x, io.xc_in, io.xc_out, io.tbias = x.data_ptr(), xc_in.data_ptr(), xc_out.data_ptr(), _dp(tbias)
    io.nbr, io.gidx, io.widx, io.patch_start = nbr.data_ptr(), gidx.data_ptr(), widx.data_ptr(), patch_start.data_ptr()
    io.num_patches, io.max_len = int(num_patches), int(max_len)
    io.scratch, io.scratch_bytes = scratch.data_ptr(), scratch.numel()
    io.sat_counter = sat_counter.data_ptr() if sat_counter is not None else None
    io.flags = int(flags)
    if logits is None:
        io.logits = io.head_w = io.head_b = io.out_idx = None
        io.num_classes = io.ld_logits = 0
    else:
        if logits.dtype != torch.float32 or head_w.dtype != torch.float32 or not head_w.is_contiguous() or (
                head_w.shape[1] != x.shape[1]) or (
                head_b is not None and head_b.dtype != torch.float32) or (out_idx is not None and out_idx.dtype != torch.int32):
            raise _lib.CdsegError("block_forward: logits / head_w / head_b are fp32 (head_w contiguous), out_idx int32")
        io.logits, io.head_w, io.head_b, io.out_idx = logits.data_ptr(), head_w.data_ptr(), _dp(head_b), _dp(out_idx)
        io.num_classes, io.ld_logits = int(head_w.shape[0]), int(logits.stride(0))
    status = _lib.load().cdseg_block_forward(desc[1], ref, _stream())
    if status == _UNSUPPORTED and logits is not None:
        return False
    check(status, "block_forward")
    return True


def stem5_ok(cout, dtype):
    """The map-free stem kernel (csrc/stem.hip) covers the shipped stems: 32 output channels, bf16."""
    return cout == 32 and is_lp(dtype)


def child_info(zcode_sorted, seg_start, m):
    """Per parent cell: (first child row << 8) | octant occupancy (children of a cell are contiguous in z-order)."""
    _need_gpu(zcode_sorted, seg_start)
    info = torch.empty(int(m), dtype=torch.int64, device=zcode_sorted.device)
    check(_lib.load().cdseg_child_info(_ptr(zcode_sorted), _ptr(seg_start), int(m), _ptr(info), _stream()), "child_info")
    return info


def stem5_pack(w):
    """(32, 125 * 8) bf16 stem weight -> LDS image of the stem kernel (built once per weight)."""
    _need_gpu(w)
    assert is_lp(w.dtype) and tuple(w.shape) == (32, 1000)
    img = _scratch(_lib.load().cdseg_stem5_wimg_bytes(), w.device)
    check(_lib.load().cdseg_stem5_pack(_ptr(w), _ptr(img), _stream()), "stem5_pack")
    return img


def stem5(x8, wimg, scale, shift, grid, cluster, parent_nbr3, cinfo, depth, out, out2=None):
    """out (n, 32) fp32 [, out2 bf16] = GELU(BN(SubMConv3d_k5(x8))) without a 125-offset kernel map (ref: ptv3.py:633-663)."""
    _need_gpu(x8, wimg, grid, cluster, parent_nbr3, cinfo, out)
    n, m = x8.shape[0], cinfo.numel()
    check(_lib.load().cdseg_stem5(_ptr(x8), _ptr(wimg), _ptr(scale), _ptr(shift), _ptr(grid), _ptr(cluster),
                                  _ptr(parent_nbr3), _ptr(cinfo), n, m, int(depth), _ptr(out), _ptr(out2), _stream()), "stem5")
    return out


def subm_conv3_ok(x):
    """The weight-stationary live-list conv (csrc/conv.hip) covers the wide bf16 stages: C = 32 / 64."""
    n = x.shape[0]  # (32-bit buffer offsets inside the kernel: larger inputs take the gathered GEMM)
    return (is_lp(x.dtype) and x.dim() == 2 and x.shape[1] in (32, 64) and x.stride(0) == x.shape[1] and
            n * 27 * 4 < 2 ** 31 and n * x.shape[1] * 2 < 2 ** 31 - 65536)


def subm_conv3_pack(w):
    """(C, 27*C) bf16 weight of a k = 3 submanifold conv -> its MFMA-fragment-order image (built once per weight)."""
    _need_gpu(w)
    c = w.shape[0]
    img = _scratch(_lib.load().cdseg_subm_conv3_wimg_bytes(c), w.device)
    check(_lib.load().cdseg_subm_conv3_pack(_ptr(w), c, _ptr(img), _stream()), "subm_conv3_pack")
    return img


def subm_conv3(x, wimg, bias, nbr_kmajor, out):
    """out (n, C) bf16 = bias + sum_o x[nbr[o]] W_o^T   (ref call sites: ptv3.py:356-362)."""
    _need_gpu(x, wimg, nbr_kmajor, out)
    n, c = x.shape
    check(_lib.load().cdseg_subm_conv3(_ptr(x), x.stride(0), _ptr(wimg), _ptr(bias), _ptr(nbr_kmajor), n, c, _ptr(out),
                                       out.stride(0), _stream()), "subm_conv3")
    return out


def subm_conv3_f32(x, wimg, bias, nbr_kmajor, out, out_scale=1.0, accumulate=False):
    """The weight-stationary conv with an fp32 output: out = (accumulate ? out : 0) + (conv + bias) * out_scale."""
    _need_gpu(x, wimg, nbr_kmajor, out)
    n, c = x.shape
    check(_lib.load().cdseg_subm_conv3_f32(_ptr(x), x.stride(0), _ptr(wimg), _ptr(bias), _ptr(nbr_kmajor), n, c, _ptr(out),
                                           out.stride(0), float(out_scale), 1 if accumulate else 0, _stream()),
          "subm_conv3_f32")
    return out


def layernorm(x, gamma, beta, out, *, eps=1e-5, res=None, colbias=None, out2=None):
    m, c = x.shape
    check(_lib.load().cdseg_layernorm(_ptr(x), dt(x), x.stride(0), _ptr(gamma), _ptr(beta), float(eps), _ptr(res),
                                      res.stride(0) if res is not None else 0, _ptr(colbias), _ptr(out), dt(out),
                                      out.stride(0), _ptr(out2), dt(out2) if out2 is not None else 0,
                                      out2.stride(0) if out2 is not None else 0, m, c, _stream()), "layernorm")
    return out


ATTN_Q_PRESCALED, ATTN_V_BF16 = 1, 2  # include/cdseg.h: producer-side preprocessing declared to cdseg_attention_ex
BLOCK_X_DEAD = 1  # include/cdseg.h: cdseg_block_io.flags / cdseg_attn_tail_rr_ex - the caller reads x no more
TAIL_AUX_X_SKIPPED, TAIL_AUX_LOGITS = 1, 2  # aux word of a tail_rr_kernel route record
_UNSUPPORTED = -4


def attention(q, k, v, q_gidx, kv_gidx, widx, patch_start, num_heads, max_len, scale, out, work=0.0, flags=0):
    """q/k/v: 2-D views (rows, H*16) of the projection buffers (any row stride); out (rows, H*16).
    flags: ATTN_Q_PRESCALED (q carries scale * log2 e: `scale` ignored) | ATTN_V_BF16 (v is bfloat16 in the half build too).
    work: algorithmic FLOPs of this launch (4 * 16 * H * sum_p L_p * kept queries of p), only used by the bench timer."""
    num_patches = patch_start.numel() - 1
    if not (q.dtype == k.dtype == out.dtype) or (v.dtype != q.dtype and not (flags & ATTN_V_BF16)):
        raise _lib.CdsegError("attention: q, k, v, out must share a dtype")
    tok = TIMER.begin("attention") if TIMER is not None else None
    check(_lib.load().cdseg_attention_ex(_ptr(q), _ptr(k), _ptr(v), q.stride(0), k.stride(0), v.stride(0), _ptr(q_gidx),
                                         _ptr(kv_gidx), _ptr(widx), _ptr(patch_start), num_patches, int(num_heads),
                                         int(max_len), float(scale), _ptr(out), out.stride(0),
                                         F32X3 if (_TLS.f32x3 and q.dtype == torch.float32) else dt(q), int(flags), _stream()),
          "attention")
    if tok is not None:
        TIMER.end(tok, work)
    return out


def segment_max(y, seg_start, m, scale, shift, act, out, out2=None):
    c = y.shape[1]
    check(_lib.load().cdseg_segment_max(_ptr(y), dt(y), y.stride(0), _ptr(seg_start), m, c, _ptr(scale), _ptr(shift),
                                        int(act), _ptr(out), out.stride(0), _ptr(out2),
                                        dt(out2) if out2 is not None else 0, out2.stride(0) if out2 is not None else 0,
                                        _stream()), "segment_max")
    return out


def pool_fused_ok(cin, cout, dtype):
    """The one-launch pooling (csrc/pool.hip) covers the wide 16-bit stages: 32 -> 64 and 64 -> 128 channels."""
    return is_lp(dtype) and (int(cin), int(cout)) in ((32, 64), (64, 128))


def pool_fused_pack(w):
    """(cout, cin) 16-bit projection weight -> its MFMA-fragment image (built once per weight)."""
    _need_gpu(w)
    cout, cin = w.shape
    lib = _lib.load()
    img = _scratch(lib.cdseg_pool_fused_img_bytes(cin, cout), w.device)
    check(lib.cdseg_pool_fused_pack(_ptr(w), cin, cout, _ptr(img), _stream()), "pool_fused_pack")
    return img


def pool_fused(x, wimg, bias, seg_start, m, scale, shift, act, out, out2=None):
    """out (m, cout) fp32 = act(scale * max over each run of round16(x W^T + bias) + shift), out2 its 16-bit copy.
    The runs cover the rows of x (seg_start[m] = x.shape[0]): the library picks its fold from x.shape[0] / m."""
    _need_gpu(x, out)
    cin, cout = x.shape[1], out.shape[1]
    check(_lib.load().cdseg_pool_fused_n(_ptr(x), x.stride(0), x.shape[0], _ptr(wimg), _ptr(bias), _ptr(seg_start), int(m),
                                         _ptr(scale), _ptr(shift), int(act), _ptr(out), out.stride(0), _ptr(out2),
                                         out2.stride(0) if out2 is not None else 0, cin, cout, _stream()), "pool_fused")
    return out


POOL_FOLD_AUTO, POOL_FOLD_WALK, POOL_FOLD_SCAN = 0, 1, 2  # include/cdseg.h cdseg_pool_fused_fold


class pool_fused_fold:
    """`with ops.pool_fused_fold(ops.POOL_FOLD_SCAN): ...` - test hook: every pool_fused launch of the process inside the block
    folds its runs the given way instead of choosing by run length (the results are the same bits either way)."""

    def __init__(self, fold):
        self.fold, self.lib = int(fold), _lib.load()

    def __enter__(self):
        self.prev = self.lib.cdseg_pool_fused_fold(self.fold)
        if self.prev < 0:
            check(self.prev, "pool_fused_fold")
        return self

    def __exit__(self, *exc):
        self.lib.cdseg_pool_fused_fold(self.prev)
        return False


def unpool_fused_ok(k_skip, k_child, c, dtype, device):
    """The one-launch unpooling (csrc/pool.hip) covers the wide 16-bit decoder stages on the GPU: skip 32 / child 64 and
    skip 64 / child 128 input channels, 64 output channels."""
    return (is_lp(dtype) and torch.device(device).type == "cuda"
            and (int(k_skip), int(k_child), int(c)) in ((32, 64, 64), (64, 128, 64)))


def unpool_fused_pack(w):
    """(64, cin) 16-bit projection weight -> its MFMA-fragment image (built once per weight)."""
    _need_gpu(w)
    cout, cin = w.shape
    lib = _lib.load()
    img = _scratch(lib.cdseg_unpool_fused_img_bytes(cin, cout), w.device)
    check(lib.cdseg_unpool_fused_pack(_ptr(w), cin, cout, _ptr(img), _stream()), "unpool_fused_pack")
    return img


def unpool_fused(skip_x, wimg_skip, bias_skip, scale_skip, shift_skip, coarse_x, wimg_child, bias_child, scale_child, shift_child,
                 seg_start, m, act, out, out2):
    """out (n, c) fp32 = s + act(scale_child * (coarse_x W_child^T + bias_child) + shift_child)[the run that holds the row],
    s = act(scale_skip * (skip_x W_skip^T + bias_skip) + shift_skip); out2 (n, c) 16-bit = s.  Runs = seg_start (m + 1)."""
    _need_gpu(skip_x, coarse_x, out, out2)
    check(_lib.load().cdseg_unpool_fused(_ptr(skip_x), skip_x.stride(0), _ptr(wimg_skip), _ptr(bias_skip), _ptr(scale_skip),
                                         _ptr(shift_skip), _ptr(coarse_x), coarse_x.stride(0), _ptr(wimg_child), _ptr(bias_child),
                                         _ptr(scale_child), _ptr(shift_child), _ptr(seg_start), int(m), int(act), _ptr(out),
                                         out.stride(0), _ptr(out2), out2.stride(0), skip_x.shape[1], coarse_x.shape[1],
                                         out.shape[1], _stream()), "unpool_fused")
    return out


def segment_mean(x, seg_start, m):
    out = torch.empty((m, x.shape[1]), dtype=torch.float32, device=x.device)
    check(_lib.load().cdseg_segment_mean(_ptr(x), x.stride(0), _ptr(seg_start), m, x.shape[1], _ptr(out),
                                         out.stride(0), _stream()), "segment_mean")
    return out


def gemv(w, b, x, act=ACT_NONE):
    n, k = w.shape
    y = torch.empty(n, dtype=torch.float32, device=w.device)
    check(_lib.load().cdseg_gemv(_ptr(w), _ptr(b), _ptr(x), n, k, int(act), _ptr(y), _stream()), "gemv")
    return y


def randn(shape, seed, offset, device, out=None):
    """out: a contiguous float32 tensor of `shape` to fill (a row slice of a larger one) instead of a fresh allocation."""
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    elif tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.CdsegError("randn: `out` is a contiguous float32 tensor of the requested shape")
    check(_lib.load().cdseg_randn(_ptr(out), out.numel(), int(seed) & (2 ** 64 - 1), int(offset), _stream()), "randn")
    return out


def cast(src, dtype):
    src = src.contiguous()
    out = torch.empty(src.shape, dtype=dtype, device=src.device)
    check(_lib.load().cdseg_cast(_ptr(src), dt(src), _ptr(out), _DT[dtype], src.numel(), _stream()), "cast")
    return out


def gather_pad_cast(src, idx, cpad, dtype):
    """(n, cin) fp32 rows gathered by idx (None = identity), zero-padded to cpad columns, cast to dtype."""
    src = src.contiguous()
    n = idx.numel() if idx is not None else src.shape[0]
    out = torch.empty((n, cpad), dtype=dtype, device=src.device)
    check(_lib.load().cdseg_gather_pad_cast(_ptr(src), src.stride(0), _ptr(idx), n, src.shape[1], int(cpad), _ptr(out),
                                            _DT[dtype], _stream()), "gather_pad_cast")
    return out


def ddim_update(xt, eps, sqrt_ab_prev, sqrt_1m_ab, sqrt_ab, sqrt_1m_ab_prev, final=False):
    out = torch.empty_like(xt)
    check(_lib.load().cdseg_ddim_update(_ptr(xt), _ptr(eps), float(sqrt_ab_prev), float(sqrt_1m_ab), float(sqrt_ab),
                                 float(sqrt_1m_ab_prev), 1 if final else 0, _ptr(out), xt.numel(), _stream()),
          "ddim_update")
    return out


def axpy(a, b, alpha):
    out = torch.empty_like(a)
    check(_lib.load().cdseg_axpy(_ptr(a), _ptr(b), float(alpha), _ptr(out), a.numel(), _stream()), "axpy")
    return out


MSI_SET, MSI_ADD, MSI_MEAN = 0, 1, 2  # cdseg_msi_step's acc_mode


def msi_step(c_xt=None, eps=None, sqrt_ab_prev=0.0, sqrt_1m_ab=0.0, sqrt_ab=1.0, sqrt_1m_ab_prev=0.0, final=False,
             acc=None, logits=None, acc_mode=MSI_ADD, scale=1.0):
    """One launch for the glue of a multi-step inference step: c_xt <- ddim_update(c_xt, eps, ...) IN PLACE (eps None: skipped)
    and acc <- logits | acc + logits | (acc + logits) * scale (acc None: skipped).  Bit-equal to ddim_update / axpy."""
    for name, a, b in (("c_xt / eps", c_xt, eps), ("acc / logits", acc, logits)):
        for t in (a, b):
            if t is not None:
                _need_gpu(t)
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise ValueError(f"msi_step: {name} must be contiguous float32 tensors")
        if a is not None and b is not None and a.numel() != b.numel():
            raise ValueError(f"msi_step: {name} differ in size ({a.numel()} / {b.numel()})")
    n_c = c_xt.numel() if c_xt is not None else (eps.numel() if eps is not None else 0)
    n_l = logits.numel() if logits is not None else (acc.numel() if acc is not None else 0)
    check(_lib.load().cdseg_msi_step(_ptr(c_xt), _ptr(eps), n_c, float(sqrt_ab_prev), float(sqrt_1m_ab), float(sqrt_ab),
                                     float(sqrt_1m_ab_prev), 1 if final else 0, _ptr(acc), _ptr(logits), n_l, int(acc_mode),
                                     float(scale), _stream()), "msi_step")


# ------------------------------------------------------------------ test-time pipeline ops
def voxelize(coord, grid_size):
    """GridSample's voxel coordinates: (grid int32 (n,3) shifted to start at 0, key int64 (n), min int32 (3))."""
    _need_gpu(coord)
    coord = coord.float().contiguous()
    n = coord.shape[0]
    grid = torch.empty((n, 3), dtype=torch.int32, device=coord.device)
    key = torch.empty(n, dtype=torch.int64, device=coord.device)
    mn = torch.empty(3, dtype=torch.int32, device=coord.device)
    check(_lib.load().cdseg_voxelize(_ptr(coord), float(grid_size), n, _ptr(grid), _ptr(key), _ptr(mn), _stream()), "voxelize")
    return grid, key, mn


def voxelize_any(coord, grid_size):
    """voxelize for float32 or float64 coordinates (GridSample after a test-time rotation sees float64)."""
    if coord.dtype != torch.float64:
        return voxelize(coord, grid_size)
    _need_gpu(coord)
    coord = coord.contiguous()
    n = coord.shape[0]
    grid = torch.empty((n, 3), dtype=torch.int32, device=coord.device)
    key = torch.empty(n, dtype=torch.int64, device=coord.device)
    mn = torch.empty(3, dtype=torch.int32, device=coord.device)
    check(_lib.load().cdseg_voxelize_f64(_ptr(coord), float(grid_size), n, _ptr(grid), _ptr(key), _ptr(mn), _stream()),
          "voxelize_f64")
    return grid, key, mn


def center_shift(coord, apply_z=True):
    """CenterShift (ref: datasets/transform.py:142-155): coord - [(xmin+xmax)/2, (ymin+ymax)/2, zmin or 0], in coord's dtype."""
    _need_gpu(coord)
    assert coord.dtype in (torch.float32, torch.float64) and coord.dim() == 2 and coord.shape[1] == 3
    coord = coord.contiguous()
    out = torch.empty_like(coord)
    ws = torch.empty(12, dtype=torch.float64, device=coord.device)
    check(_lib.load().cdseg_center_shift(_ptr(coord), 1 if coord.dtype == torch.float64 else 0, coord.shape[0],
                                         1 if apply_z else 0, _ptr(out), _ptr(ws), _stream()), "center_shift")
    return out


def tta_apply(xyz, rot=None, scale=None, flip=False):
    """One test-time augmentation of an (n,3) float32 array (ref: transform.py:259-328).  rot (3x3 nested floats):
    float64 result (xyz @ rot^T) [* scale]; else flip: float32 result with x, y negated; neither: xyz itself."""
    _need_gpu(xyz)
    xyz = xyz.float().contiguous()
    n = xyz.shape[0]
    if rot is None and not flip:
        return xyz
    if rot is not None:
        r = (ctypes.c_double * 9)(*[float(v) for row in rot for v in row])
        out = torch.empty((n, 3), dtype=torch.float64, device=xyz.device)
        check(_lib.load().cdseg_tta_apply(_ptr(xyz), n, r, float(scale if scale is not None else 1.0),
                                          1 if scale is not None else 0, 0, _ptr(out), _stream()), "tta_apply")
        return out
    out = torch.empty_like(xyz)
    check(_lib.load().cdseg_tta_apply(_ptr(xyz), n, None, 1.0, 0, 1, _ptr(out), _stream()), "tta_apply")
    return out


def div_add(x, div, add):
    """x / div + add in float32 (NormalizeColor = (color, 127.5, -1), ref: transform.py:113-117)."""
    _need_gpu(x)
    x = x.float().contiguous()
    out = torch.empty_like(x)
    check(_lib.load().cdseg_div_add(_ptr(x), float(div), float(add), x.numel(), _ptr(out), _stream()), "div_add")
    return out


def collect_feat(a, b):
    """Collect(feat_keys=(a, b)): cat([a.float(), b.float()], 1) (ref: transform.py:46-49); b float32 or float64."""
    _need_gpu(a, b)
    a = a.float().contiguous()
    b = b.contiguous()
    n = a.shape[0]
    out = torch.empty((n, a.shape[1] + b.shape[1]), dtype=torch.float32, device=a.device)
    check(_lib.load().cdseg_collect_feat(_ptr(a), a.shape[1], _ptr(b), 1 if b.dtype == torch.float64 else 0, b.shape[1], n,
                                         _ptr(out), _stream()), "collect_feat")
    return out


def max_run(seg_start, m):
    out = torch.empty(1, dtype=torch.int32, device=seg_start.device)
    check(_lib.load().cdseg_max_run(_ptr(seg_start), int(m), _ptr(out), _stream()), "max_run")
    return out


def fragment_select(idx_sort, seg_start, m, frag):
    out = torch.empty(int(m), dtype=torch.int32, device=idx_sort.device)
    check(_lib.load().cdseg_fragment_select(_ptr(idx_sort), _ptr(seg_start), int(m), int(frag), _ptr(out), _stream()),
          "fragment_select")
    return out


def softmax_vote(logits, idx, pred):
    check(_lib.load().cdseg_softmax_vote(_ptr(logits), logits.stride(0), _ptr(idx), logits.shape[0], logits.shape[1], _ptr(pred),
                                  pred.stride(0), _stream()), "softmax_vote")
    return pred


def argmax_rows(x):
    out = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    check(_lib.load().cdseg_argmax_rows(_ptr(x), x.stride(0), x.shape[0], x.shape[1], _ptr(out), _stream()), "argmax_rows")
    return out


def fragments_build(idx_sort, seg_start, m, frags, grid, feat, coord, center_shift=False):
    """All ``frags`` fragments of one augmented scan as dense arrays, in launches that do not depend on ``frags``:
    -> (index (F,m) int32, coord (F,m,3) float32, grid_coord (F,m,3) int32, feat (F,m,C) float32).  grid (n,3) int32,
    feat (n,C) float32, coord (n,3) float32 / float64; center_shift: the per-fragment CenterShift(apply_z=False) in
    coord's precision before the one rounding to float32 (include/cdseg.h)."""
    _need_gpu(idx_sort, seg_start, grid, feat, coord)
    lib = _lib.load()
    assert grid.dtype == torch.int32 and feat.dtype == torch.float32 and coord.dtype in (torch.float32, torch.float64)
    assert feat.dim() == 2 and coord.shape == grid.shape == (feat.shape[0], 3)
    grid, feat, coord = grid.contiguous(), feat.contiguous(), coord.contiguous()
    m, frags, n, c, dev = int(m), int(frags), feat.shape[0], feat.shape[1], feat.device
    index = torch.empty((frags, m), dtype=torch.int32, device=dev)
    coord_out = torch.empty((frags, m, 3), dtype=torch.float32, device=dev)
    grid_out = torch.empty((frags, m, 3), dtype=torch.int32, device=dev)
    feat_out = torch.empty((frags, m, c), dtype=torch.float32, device=dev)
    ws = workspace(lib.cdseg_fragments_build_ws_bytes(frags), dev) if center_shift else None
    check(lib.cdseg_fragments_build(_ptr(idx_sort), _ptr(seg_start), m, frags, n, _ptr(grid), _ptr(feat), c, _ptr(coord),
                                    1 if coord.dtype == torch.float64 else 0, 1 if center_shift else 0, _ptr(index),
                                    _ptr(grid_out), _ptr(feat_out), _ptr(coord_out), _ptr(ws), 0 if ws is None else ws.numel(),
                                    _stream()), "fragments_build")
    return index, coord_out, grid_out, feat_out


def softmax_vote_fragments(logits, index, pred):
    """pred[index[f][v]] += softmax(logits[f m + v]) for the k = index.shape[0] collated fragments, f ascending, one launch;
    bit-equal to k successive softmax_vote calls on fragments_build's index rows."""
    _need_gpu(logits, index, pred)
    k, m = index.shape
    assert index.dtype == torch.int32 and index.is_contiguous() and logits.shape[0] == k * m
    assert logits.dtype == pred.dtype == torch.float32 and logits.stride(1) == 1 and pred.stride(1) == 1
    assert pred.shape[1] == logits.shape[1]
    check(_lib.load().cdseg_softmax_vote_fragments(_ptr(logits), logits.stride(0), _ptr(index), m, k, logits.shape[1], _ptr(pred),
                                                   pred.stride(0), pred.shape[0], _stream()), "softmax_vote_fragments")
    return pred


def voxel_inverse(idx_sort, cluster):
    """GridSample(return_inverse=True): inverse (n,) int32 with inverse[idx_sort[j]] = cluster[j]."""
    _need_gpu(idx_sort, cluster)
    n = idx_sort.numel()
    assert idx_sort.dtype == cluster.dtype == torch.int32 and cluster.numel() >= n
    out = torch.empty(n, dtype=torch.int32, device=idx_sort.device)
    check(_lib.load().cdseg_voxel_inverse(_ptr(idx_sort), _ptr(cluster), n, _ptr(out), _stream()), "voxel_inverse")
    return out


def knn1(ref_xyz, ref_offset, qry_xyz, qry_offset, origin, cell, want_dist=False):
    """Exact nearest reference point (same batch element) of every query.  offsets: int32 cumulative ends."""
    lib = _lib.load()
    _need_gpu(ref_xyz, qry_xyz)
    ref_xyz, qry_xyz = ref_xyz.float().contiguous(), qry_xyz.float().contiguous()
    n, m = ref_xyz.shape[0], qry_xyz.shape[0]
    idx = torch.empty(m, dtype=torch.int32, device=qry_xyz.device)
    d2 = torch.empty(m, dtype=torch.float32, device=qry_xyz.device) if want_dist else None
    ws = workspace(lib.cdseg_knn1_ws_bytes(n), qry_xyz.device)
    org = (ctypes.c_float * 3)(*[float(v) for v in origin])
    check(lib.cdseg_knn1(_ptr(ref_xyz), _ptr(ref_offset), n, _ptr(qry_xyz), _ptr(qry_offset), m, ref_offset.numel(), org,
                         float(cell), _ptr(idx), _ptr(d2), _ptr(ws), ws.numel(), _stream()), "knn1")
    return (idx, d2) if want_dist else idx


def knn(k, ref_xyz, ref_offset, qry_xyz=None, qry_offset=None, origin=None, cell=None):
    """pointops.knn_query(k, xyz, offset, new_xyz, new_offset) (ref: libs/pointops/functions/query.py:7-24): the k nearest
    reference points (same batch element) of every query -> (idx (m, k) int32 with -1 placeholders, dist (m, k) float32 =
    EUCLIDEAN distances like the reference's wrapper, placeholders sqrt(1e10)).  Ascending by (distance, index).
    origin / cell default to the reference points' minimum and a cell that holds ~2 points on average (one host read)."""
    lib = _lib.load()
    _need_gpu(ref_xyz)
    if qry_xyz is None:
        qry_xyz, qry_offset = ref_xyz, ref_offset
    ref_xyz, qry_xyz = ref_xyz.float().contiguous(), qry_xyz.float().contiguous()
    ref_offset, qry_offset = ref_offset.to(torch.int32).contiguous(), qry_offset.to(torch.int32).contiguous()
    n, m = ref_xyz.shape[0], qry_xyz.shape[0]
    if origin is None or cell is None:
        lo, hi = ref_xyz.min(0).values, ref_xyz.max(0).values
        ext = (hi - lo).clamp_min(1e-6).cpu().tolist()
        origin = lo.cpu().tolist()
        # surface-like clouds: cells of side s hold ~ n s^2 / area points; aim at ~2 per cell
        area = max(ext[0] * ext[1], ext[0] * ext[2], ext[1] * ext[2])
        cell = max((2.0 * area / max(n, 1)) ** 0.5, max(ext) / ((1 << 20) - 2))
    idx = torch.empty((m, int(k)), dtype=torch.int32, device=qry_xyz.device)
    d2 = torch.empty((m, int(k)), dtype=torch.float32, device=qry_xyz.device)
    ws = workspace(lib.cdseg_knn1_ws_bytes(n), qry_xyz.device)
    org = (ctypes.c_float * 3)(*[float(v) for v in origin])
    check(lib.cdseg_knn(_ptr(ref_xyz), _ptr(ref_offset), n, _ptr(qry_xyz), _ptr(qry_offset), m, ref_offset.numel(), int(k), org,
                        float(cell), _ptr(idx), _ptr(d2), _ptr(ws), ws.numel(), _stream()), "knn")
    return idx, torch.sqrt(d2)


def iou_counts(pred, target, num_classes, ignore_index=-1, pred_idx=None):
    """(3, K) int64: intersection, prediction and target counts (rows with target == ignore_index dropped)."""
    out = torch.empty((3, num_classes), dtype=torch.int64, device=pred.device)
    check(_lib.load().cdseg_iou_counts(_ptr(pred), _ptr(pred_idx), _ptr(target), target.numel(), int(num_classes),
                                        int(ignore_index), _ptr(out), _stream()), "iou_counts")
    return out


# ------------------------------------------------------------------ reference-shaped composites
def serialization(grid_coord, batch, orders=("z", "z-trans", "hilbert", "hilbert-trans"), depth=None):
    """Point.serialization before the shuffle (structure.py:47-93): code, order, inverse as (k, N) int64
    in the caller's point order - the drop-in for the reference's encode + argsort + scatter_."""
    _need_gpu(grid_coord, batch)
    if depth is None:
        depth = int(grid_max(grid_coord).item()).bit_length()
    codes, orders_, inverses = [], [], []
    nb = int(batch.max().item()) + 1 if batch.numel() else 1
    end_bit = 3 * depth + max(1, nb.bit_length())
    for o in orders:
        c = encode(grid_coord, batch, depth, o)
        _, perm = sort_pairs(c, None, end_bit=min(64, end_bit))
        codes.append(c)
        orders_.append(widen(perm))
        inverses.append(widen(invert_perm(perm)))
    return torch.stack(codes), torch.stack(orders_), torch.stack(inverses), depth


# ------------------------------------------------------------------ training path (csrc/train.hip)
def attention_bwd(q, k, v, q_gidx, kv_gidx, widx, patch_start, patch_start_host, num_heads, scale, dout, dq, dk, dv):
    """Gradients of `attention`: fp32 dq / dk / dv (views of zero-initialised buffers, any row stride) += at the gathered
    rows.  q / k / v / dout share a dtype: fp32 (exact-fp32 kernels), or the active build's 16-bit type (the recompute-P
    backward of the 16-bit forward on the 16-bit matrix pipe; dout is used as it comes: an inf stays an inf).
    patch_start_host: the same patch table as Python ints (tile count of the launch)."""
    _need_gpu(q, dout)
    if not (q.dtype == k.dtype == v.dtype == dout.dtype):
        raise _lib.CdsegError("attention_bwd: q, k, v, dout must share a dtype")
    if not (dq.dtype == dk.dtype == dv.dtype == torch.float32):
        raise _lib.CdsegError("attention_bwd: dq, dk, dv are fp32 (accumulated into)")
    code = dt(q)  # (a 16-bit tensor of the other build's type raises here)
    ps = [int(x) for x in patch_start_host]
    num_patches = len(ps) - 1
    max_len = max((ps[i + 1] - ps[i] for i in range(num_patches)), default=0)
    if max_len > 1024:
        raise _lib.CdsegError("attention_bwd: a patch holds at most 1024 slots (the patch-head lives in LDS, like the forward)")
    per16 = 16 // q.element_size()
    for t, ld in ((q, q.stride(0)), (k, k.stride(0)), (v, v.stride(0)), (dout, dout.stride(0))):
        if ld % per16 or t.data_ptr() % 16 or t.stride(1) != 1:
            raise _lib.CdsegError("attention_bwd: rows must be 16-byte aligned (float4 operand loads)" if per16 == 4 else
                                  "attention_bwd: rows must be 16-byte aligned (eight 16-bit values per operand load)")
    for t in (dq, dk, dv):
        if t.stride(0) % 4 or t.data_ptr() % 16 or t.stride(1) != 1:
            raise _lib.CdsegError("attention_bwd: gradient rows must be 16-byte aligned")
    lib = _lib.load()
    ws = _scratch(max(1, lib.cdseg_attention_bwd_ws_bytes(ps[-1], int(num_heads))), q.device)
    check(lib.cdseg_attention_bwd(_ptr(q), _ptr(k), _ptr(v), q.stride(0), k.stride(0), v.stride(0), _ptr(q_gidx),
                                  _ptr(kv_gidx), _ptr(widx), _ptr(patch_start), num_patches, int(num_heads), ps[-1], max(1, max_len),
                                  float(scale), _ptr(dout), dout.stride(0), _ptr(dq), _ptr(dk), _ptr(dv), dq.stride(0),
                                  dk.stride(0), dv.stride(0), code, _ptr(ws), ws.numel(), _stream()), "attention_bwd")


# ---- dropout (include/cdseg.h "dropout"; csrc/attention_drop.hip, the mask variants of csrc/train.hip)
_U64 = 2 ** 64 - 1


def _drop_rate(what, rate):
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise _lib.CdsegError(f"{what}: rate must lie in [0, 1), got {rate!r}")
    return rate


def dropout_keep(rate):
    """The effective keep probability T / 256 of a dropout rate: T = floor(256 (1 - rate) + 1/2), at least 1 (8-bit
    granularity; kept values are divided by it)."""
    rate = _drop_rate("dropout_keep", rate)
    return max(1, int(math.floor(256.0 * (1.0 - rate) + 0.5))) / 256.0


def attention_drop(q, k, v, q_gidx, kv_gidx, widx, patch_start, num_heads, max_len, scale, out, rate, seed, offset):
    """`attention` with dropout on the probabilities: out = ((M / keep) o softmax(scale q k^T)) v, M the library's mask of
    the site (seed, offset) at `rate`.  fp32, or the active build's 16-bit type (q not prescaled, v of the same type)."""
    _need_gpu(q, out)
    rate = _drop_rate("attention_drop", rate)
    if not (q.dtype == k.dtype == v.dtype == out.dtype):
        raise _lib.CdsegError("attention_drop: q, k, v, out must share a dtype")
    code = dt(q)
    check(_lib.load().cdseg_attention_drop(_ptr(q), _ptr(k), _ptr(v), q.stride(0), k.stride(0), v.stride(0), _ptr(q_gidx),
                                           _ptr(kv_gidx), _ptr(widx), _ptr(patch_start), patch_start.numel() - 1, int(num_heads),
                                           int(max_len), float(scale), _ptr(out), out.stride(0), code, rate, int(seed) & _U64,
                                           int(offset) & _U64, _stream()), "attention_drop")
    return out


def attention_drop_bwd(q, k, v, q_gidx, kv_gidx, widx, patch_start, patch_start_host, num_heads, scale, dout, dq, dk, dv, rate,
                       seed, offset):
    """Gradients of `attention_drop` at the same (rate, seed, offset); everything else as `attention_bwd`."""
    _need_gpu(q, dout)
    rate = _drop_rate("attention_drop_bwd", rate)
    if not (q.dtype == k.dtype == v.dtype == dout.dtype):
        raise _lib.CdsegError("attention_drop_bwd: q, k, v, dout must share a dtype")
    if not (dq.dtype == dk.dtype == dv.dtype == torch.float32):
        raise _lib.CdsegError("attention_drop_bwd: dq, dk, dv are fp32 (accumulated into)")
    code = dt(q)
    ps = [int(x) for x in patch_start_host]
    num_patches = len(ps) - 1
    max_len = max((ps[i + 1] - ps[i] for i in range(num_patches)), default=0)
    lib = _lib.load()
    ws = _scratch(max(1, lib.cdseg_attention_bwd_ws_bytes(ps[-1], int(num_heads))), q.device)
    check(lib.cdseg_attention_drop_bwd(_ptr(q), _ptr(k), _ptr(v), q.stride(0), k.stride(0), v.stride(0), _ptr(q_gidx),
                                       _ptr(kv_gidx), _ptr(widx), _ptr(patch_start), num_patches, int(num_heads), ps[-1],
                                       max(1, max_len), float(scale), _ptr(dout), dout.stride(0), _ptr(dq), _ptr(dk), _ptr(dv),
                                       dq.stride(0), dk.stride(0), dv.stride(0), code, _ptr(ws), ws.numel(), rate,
                                       int(seed) & _U64, int(offset) & _U64, _stream()), "attention_drop_bwd")


def dropout(x, rate, seed, offset, out=None):
    """out = x o M / keep on a 2-D fp32 tensor (any row stride; out may be x), M the library's element mask of the site
    (seed, offset).  Its own backward: dropout(dy, rate, seed, offset)."""
    _need_gpu(x)
    rate = _drop_rate("dropout", rate)
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    if x.dim() != 2 or out.shape != x.shape or x.dtype != torch.float32 or out.dtype != torch.float32:
        raise _lib.CdsegError("dropout: x and out are fp32 (m, c) tensors of one shape")
    if x.shape[1] > 1 and (x.stride(1) != 1 or out.stride(1) != 1):
        raise _lib.CdsegError("dropout: rows must be contiguous")
    check(_lib.load().cdseg_dropout(_ptr(x), x.stride(0), _ptr(out), out.stride(0), x.shape[0], x.shape[1], rate,
                                    int(seed) & _U64, int(offset) & _U64, _stream()), "dropout")
    return out


def layernorm_bwd(x, gamma, dy, dx, accumulate=False, eps=1e-5, dgamma=None, dbeta=None, deterministic=False):
    """dx (=, or += with accumulate) of y = LayerNorm(x) * gamma + beta; fp32.  deterministic: dgamma / dbeta are summed in a
    fixed order (block partials in a workspace from torch's allocator, added by ascending block index; rows up to 512 wide)."""
    _need_gpu(x, dy)
    lib = _lib.load()
    if deterministic:
        ws = _scratch(max(16, lib.cdseg_layernorm_bwd_det_ws_bytes(x.shape[0], x.shape[1])), x.device)
        check(lib.cdseg_layernorm_bwd_det(_ptr(x), x.stride(0), _ptr(gamma), float(eps), _ptr(dy), dy.stride(0), _ptr(dx),
                                          dx.stride(0), int(bool(accumulate)), _ptr(dgamma), _ptr(dbeta), x.shape[0],
                                          x.shape[1], _ptr(ws), ws.numel(), _stream()), "layernorm_bwd (deterministic)")
        return dx
    check(lib.cdseg_layernorm_bwd(_ptr(x), x.stride(0), _ptr(gamma), float(eps), _ptr(dy), dy.stride(0), _ptr(dx),
                                  dx.stride(0), int(bool(accumulate)), _ptr(dgamma), _ptr(dbeta), x.shape[0],
                                  x.shape[1], _stream()), "layernorm_bwd")
    return dx


def gelu_bwd(u, dy):
    """dy * GELU'(u) on the pre-activation u (erf form); fp32, contiguous."""
    _need_gpu(u, dy)
    dx = torch.empty_like(u)
    check(_lib.load().cdseg_gelu_bwd(_ptr(u), _ptr(dy), _ptr(dx), u.numel(), _stream()), "gelu_bwd")
    return dx


def _wgrad_operands(what, x, dy, dw, db):
    """fp32 operands -> False; the active build's 16-bit type -> True (x and dy 16-byte aligned rows); dw / db are fp32."""
    if x.dtype != dy.dtype:
        raise _lib.CdsegError(f"{what}: x and dy must share a dtype")
    if dw.dtype != torch.float32 or (db is not None and db.dtype != torch.float32):
        raise _lib.CdsegError(f"{what}: dw, db are fp32 (accumulated into)")
    if x.dtype == torch.float32:
        return False
    dt(x)  # (a 16-bit tensor of the other build's type raises here)
    for t in (x, dy):
        if t.stride(0) % 8 or t.data_ptr() % 16:
            raise _lib.CdsegError(f"{what}: rows must be 16-byte aligned (eight 16-bit values per operand load)")
    return True


def det_kw(deterministic):
    """Keyword of the gradient reductions (`linear_wgrad`, `conv_wgrad`, `layernorm_bwd`): passed only when the fixed summation
    order is asked for, so that the default call is what it was."""
    return {"deterministic": True} if deterministic else {}


class WgradPartition(tuple):
    """(rows_per_split, splits) of a weight-gradient launch: split s covers rows s * rows_per_split .. (the last may be shorter)."""
    __slots__ = ()
    rows_per_split = property(lambda self: self[0])
    splits = property(lambda self: self[1])


def wgrad_partition(m, n, k, kvol=1, dtype=torch.float32):
    """Row partition of the weight-gradient launch for dy (m, n), x (., k), kvol kernel offsets (1: the Linear form) and operands
    of `dtype` (fp32, or a 16-bit type): a function of the shape only (host code, no GPU needed, the same in both builds)."""
    rows, splits = ctypes.c_long(0), ctypes.c_int(0)
    code = F32 if dtype == torch.float32 else BF16
    check(_lib.load().cdseg_wgrad_partition(int(m), int(n), int(k), int(kvol), code, ctypes.byref(rows), ctypes.byref(splits)),
          "wgrad_partition")
    return WgradPartition((rows.value, splits.value))


def _wgrad_ws(lib, m, n, k, kvol, lp, device):
    nbytes = lib.cdseg_wgrad_det_ws_bytes(int(m), int(n), int(k), int(kvol), BF16 if lp else F32)
    return _scratch(max(16, nbytes), device)


def linear_wgrad(x, dy, dw, db=None, xidx=None, deterministic=False):
    """dw (N, K view, any row stride) += dy^T x[xidx or arange] and db (N) += column sums of dy (cdseg_linear_wgrad).
    xidx (M) int32 with -1 = no row: one kernel offset of a submanifold conv.  x and dy share a dtype: fp32, or the active
    build's 16-bit type (cdseg_linear_wgrad16: exact products, fp32 sums); dw / db are fp32 either way.
    deterministic: the same kernels with a fixed summation order (cdseg_linear_wgrad_det: the row splits of `wgrad_partition`
    leave partial tiles in a workspace from torch's allocator, a second launch adds them by ascending split index)."""
    _need_gpu(x, dy, dw)
    lp = _wgrad_operands("linear_wgrad", x, dy, dw, db)
    assert dy.stride(1) == 1 and x.stride(1) == 1 and dw.stride(1) == 1
    m, n = dy.shape
    k = x.shape[1]
    assert tuple(dw.shape) == (n, k) and (xidx is None or (xidx.dtype == torch.int32 and xidx.numel() == m))
    lib = _lib.load()
    if deterministic:
        ws = _wgrad_ws(lib, m, n, k, 1, lp, dw.device)
        check(lib.cdseg_linear_wgrad_det(_ptr(x), x.stride(0), _ptr(xidx), _ptr(dy), dy.stride(0), m, k, n, _ptr(dw), dw.stride(0),
                                         _ptr(db), BF16 if lp else F32, _ptr(ws), ws.numel(), _stream()), "linear_wgrad (deterministic)")
        return dw
    fn = lib.cdseg_linear_wgrad16 if lp else lib.cdseg_linear_wgrad
    check(fn(_ptr(x), x.stride(0), _ptr(xidx), _ptr(dy), dy.stride(0), m, k, n, _ptr(dw), dw.stride(0), _ptr(db), _stream()),
          "linear_wgrad")
    return dw


def conv_wgrad(x, nbr_kmajor, dy, dw3, db=None, deterministic=False):
    """dw3 (Cout, kvol, Cin) += the weight gradient of a submanifold conv over all kernel offsets (one launch), db += the
    bias gradient; nbr_kmajor (kvol, M) int32 offset-major kernel map.  fp32 (cdseg_conv_wgrad), or x and dy of the active
    build's 16-bit type with fp32 dw3 / db (cdseg_conv_wgrad16).  deterministic: as in `linear_wgrad` (cdseg_conv_wgrad_det)."""
    _need_gpu(x, dy, dw3)
    lp = _wgrad_operands("conv_wgrad", x, dy, dw3, db)
    kvol, m = nbr_kmajor.shape
    cout, kv, cin = dw3.shape
    assert kv == kvol and dw3.is_contiguous() and dy.stride(1) == 1 and x.stride(1) == 1
    assert nbr_kmajor.dtype == torch.int32 and nbr_kmajor.is_contiguous() and dy.shape == (m, cout) and x.shape[1] == cin
    lib = _lib.load()
    if deterministic:
        ws = _wgrad_ws(lib, m, cout, cin, kvol, lp, dw3.device)
        check(lib.cdseg_conv_wgrad_det(_ptr(x), x.stride(0), _ptr(nbr_kmajor), kvol, _ptr(dy), dy.stride(0), m, cin, cout, _ptr(dw3),
                                       _ptr(db), BF16 if lp else F32, _ptr(ws), ws.numel(), _stream()), "conv_wgrad (deterministic)")
        return dw3
    fn = lib.cdseg_conv_wgrad16 if lp else lib.cdseg_conv_wgrad
    check(fn(_ptr(x), x.stride(0), _ptr(nbr_kmajor), kvol, _ptr(dy), dy.stride(0), m, cin, cout, _ptr(dw3), _ptr(db), _stream()),
          "conv_wgrad")
    return dw3


def segment_sum(src, seg_start, m):
    """out (m, C) fp32: out[j] = sum of src rows seg_start[j] .. seg_start[j + 1] - 1, added in ascending row order
    (cdseg_segment_sum): the backward of a gather whose duplicates are contiguous, without atomics."""
    _need_gpu(src, seg_start)
    assert src.dtype == torch.float32 and src.stride(1) == 1 and seg_start.dtype == torch.int32 and seg_start.numel() >= m + 1
    out = torch.empty((m, src.shape[1]), dtype=torch.float32, device=src.device)
    check(_lib.load().cdseg_segment_sum(_ptr(src), src.stride(0), _ptr(seg_start), int(m), src.shape[1], _ptr(out), out.stride(0),
                                        _stream()), "segment_sum")
    return out


# ------------------------------------------------------------------ native training Block (csrc/trainblock.hip)
TB_PARAMS = 18                      # parameter tensors of a Block, in nn.Module order (include/cdseg.h CDSEG_TB_*)
TB_MATRICES = (0, 2, 8, 10, 14, 16)  # conv, cpe Linear, qkv, proj, fc1, fc2: the six that have 16-bit / transposed forms


class TrainBlock:
    """One Block's descriptor for the native training executor: the ctypes struct, everything it points to (kept alive here),
    the library build its 16-bit tensors belong to and the persistent derived-weights buffer."""

    def __init__(self, params, heads, attn_scale, eps, mm_variant, attn_variant, deterministic, shadows=None):
        params = list(params)
        if len(params) != TB_PARAMS:
            raise _lib.CdsegError(f"a Block has {TB_PARAMS} parameter tensors, got {len(params)}")
        _need_gpu(*params)
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.CdsegError("train_block: parameters are contiguous float32 tensors")
        if mm_variant is not None and attn_variant is not None and mm_variant != attn_variant:
            raise _lib.CdsegError("train_block: one 16-bit type per Block")
        self.variant = mm_variant or attn_variant  # the build whose 16-bit type the Block uses (None: exact fp32)
        self.mm_lp, self.attn_lp, self.deterministic = mm_variant is not None, attn_variant is not None, bool(deterministic)
        self.params = params
        self.shadows = [None] * len(TB_MATRICES) if shadows is None else list(shadows)
        self.channels, self.hidden, self.heads = params[2].shape[0], params[14].shape[0], int(heads)
        d = self.desc = _lib.TrainBlockDesc()
        d.channels, d.heads, d.hidden = self.channels, self.heads, self.hidden
        d.attn_scale = float(attn_scale)
        d.eps_cpe, d.eps_norm1, d.eps_norm2 = (float(e) for e in eps)
        d.mm_dtype, d.attn_dtype, d.deterministic = (BF16 if self.mm_lp else F32), (BF16 if self.attn_lp else F32), int(self.deterministic)
        for i, p in enumerate(params):
            d.param[i] = p.data_ptr()
        for i, s in enumerate(self.shadows):
            if s is not None and (not self.mm_lp or s.dtype != LP_DTYPES[self.variant] or not s.is_contiguous()):
                raise _lib.CdsegError("train_block: a shadow copy is a contiguous tensor of the Block's 16-bit type")
            d.shadow16[i] = None if s is None else s.data_ptr()
        self.ref = ctypes.byref(d)
        self.io = _lib.TrainBlockIO()
        self.io_ref = ctypes.byref(self.io)
        self.derived_bytes = train_block_bytes(self, 0, 0)[2]
        self.derived = _scratch(self.derived_bytes, params[0].device)
        d.derived, d.derived_bytes = self.derived.data_ptr(), self.derived_bytes
        offs = (ctypes.c_size_t * TB_PARAMS)()
        check(self.lib().cdseg_train_block_grad_offsets(self.ref, offs), "train_block_grad_offsets")
        self.grad_offsets = [int(o) for o in offs]

    def lib(self):
        return _lib.load(self.variant)


def train_block_bytes(tb, n, slots):
    """(tape, scratch, derived, grads) bytes of a Block for n rows and `slots` padded attention slots: host code, a function of
    the shape only, each a multiple of 256."""
    out = [ctypes.c_size_t(0) for _ in range(4)]
    check(tb.lib().cdseg_train_block_bytes(tb.ref, int(n), int(slots), *[ctypes.byref(o) for o in out]), "train_block_bytes")
    return tuple(int(o.value) for o in out)


def train_block_grad_views(tb, slab):
    """The 18 parameter gradients as fp32 views of the gradient slab (uint8), in parameter order, shaped like the parameters."""
    views = []
    for p, off in zip(tb.params, tb.grad_offsets):
        views.append(slab[off:off + 4 * p.numel()].view(torch.float32).view(p.shape))
    return views


def train_block_derived_views(tb):
    """The derived-weights buffer as tensors, the layout of csrc/trainblock.hip restated (every piece starts at a multiple of
    256 bytes, in the order of TB_MATRICES): [(transposed weight, 16-bit forward weight or None)] - (in, out) for a Linear,
    (cin, 27 * cout) for the conv's data-gradient kernel; 16-bit tensors when the products are 16 bit."""
    dtype = LP_DTYPES[tb.variant] if tb.mm_lp else torch.float32
    esz = 2 if tb.mm_lp else 4
    off, out = 0, []

    def take(shape, dt_, e):
        nonlocal off
        off = (off + 255) // 256 * 256
        nbytes = e * shape[0] * shape[1]
        v = tb.derived[off:off + nbytes].view(dt_).view(shape)
        off += nbytes
        return v

    for i in TB_MATRICES:
        w = tb.params[i]
        o, k = w.shape[0], w.numel() // w.shape[0]
        t = take((k // 27, 27 * o) if w.dim() == 5 else (k, o), dtype, esz)
        out.append((t, take((o, k), dtype, 2) if tb.mm_lp else None))
    return out


def train_block_prepare(tb):
    """Fill the Block's derived-weights buffer (transposed Linear weights, the conv's data-gradient kernel, 16-bit forms): one
    launch; once per weight version."""
    check(tb.lib().cdseg_train_block_prepare(tb.ref, _stream()), "train_block_prepare")


def _train_block_io(tb, n, x_in, x_conv, t_rows, scene_offs, mask1, mask2, nbr, gidx, widx, patch_start, patch_start_host, tape,
                    scratch, x_out, rows=None):
    _need_gpu(x_in, x_conv, tape, scratch)
    for t in (x_in, x_conv, x_out, t_rows, mask1, mask2):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.CdsegError("train_block: activations, masks and timestep rows are contiguous float32 tensors")
    ps = [int(v) for v in patch_start_host]
    io = tb.io
    io.n = int(n)
    io.x_in, io.x_conv, io.t_rows, io.scene_offs = x_in.data_ptr(), x_conv.data_ptr(), _dp(t_rows), _dp(scene_offs)
    io.num_scenes = 0 if t_rows is None else int(t_rows.shape[0])
    io.mask1, io.mask2 = _dp(mask1), _dp(mask2)
    io.nbr, io.gidx, io.widx, io.patch_start = nbr.data_ptr(), gidx.data_ptr(), widx.data_ptr(), patch_start.data_ptr()
    io.num_patches = len(ps) - 1
    io.max_len = max((ps[i + 1] - ps[i] for i in range(len(ps) - 1)), default=0)
    io.num_slots = ps[-1]
    io.tape, io.tape_bytes = tape.data_ptr(), tape.numel()
    io.scratch, io.scratch_bytes = scratch.data_ptr(), scratch.numel()
    io.x_out = _dp(x_out)
    if rows is None:
        io.n_conv, io.row_vox, io.row_start = 0, None, None
    else:  # the row level of a Mix3D batch (engine.RowLevel): nbr describes the row_start.numel() - 1 voxels
        row_vox, row_start = rows
        if (row_vox.dtype != torch.int32 or row_start.dtype != torch.int32 or not row_vox.is_contiguous() or not row_start.is_contiguous()
                or row_vox.numel() != int(n) or nbr.shape[-1] != row_start.numel() - 1):
            raise _lib.CdsegError("train_block: rows = (row_vox (n), row_start (voxels + 1)) contiguous int32, nbr over the voxels")
        io.n_conv, io.row_vox, io.row_start = row_start.numel() - 1, row_vox.data_ptr(), row_start.data_ptr()
    return tb.io_ref


def train_block_forward(tb, n, x_in, x_conv, t_rows, scene_offs, mask1, mask2, nbr, gidx, widx, patch_start, patch_start_host,
                        tape, scratch, x_out, rows=None):
    """One Block of the training forward on the native executor: every launch issued by the library, one host call.  x_conv is
    what the CPE conv reads (may be x_in); t_rows (B, C) with scene_offs (B + 1) int32: the per-scene timestep rows; mask1 /
    mask2 (n): stochastic-depth row masks already divided by the keep probability; tape (uint8) keeps what the backward reads.
    rows = (row_vox (n), row_start (V + 1)) int32: the n rows are the points of V voxels (engine.RowLevel), nbr is the map of the
    V voxels, the CPE runs on the first row of every voxel and every row adds its voxel's term."""
    ref = _train_block_io(tb, n, x_in, x_conv, t_rows, scene_offs, mask1, mask2, nbr, gidx, widx, patch_start, patch_start_host,
                          tape, scratch, x_out, rows)
    check(tb.lib().cdseg_train_block_forward(tb.ref, ref, _stream()), "train_block_forward")
    return x_out


def train_block_backward(tb, n, x_in, x_conv, t_rows, scene_offs, mask1, mask2, nbr, gidx, widx, patch_start, patch_start_host,
                         tape, scratch, x_out, dy, dx_in, dx_conv, dt_rows, slab, rows=None):
    """Backward of `train_block_forward` (same arguments, the forward's tape): dx_in, dx_conv (None when x_conv is x_in: the conv's
    data gradient is added into dx_in), dt_rows (with t_rows) and the gradient slab (zeroed here by one memset;
    `train_block_grad_views`)."""
    ref = _train_block_io(tb, n, x_in, x_conv, t_rows, scene_offs, mask1, mask2, nbr, gidx, widx, patch_start, patch_start_host,
                          tape, scratch, x_out, rows)
    _need_gpu(dy, dx_in, slab)
    for t in (dy, dx_in, dx_conv, dt_rows):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.CdsegError("train_block: gradients are contiguous float32 tensors")
    check(tb.lib().cdseg_train_block_backward(tb.ref, ref, _ptr(dy), _ptr(dx_in), _ptr(dx_conv), _ptr(dt_rows), _ptr(slab),
                                              _stream()), "train_block_backward")


def gather_first(x, row_start, variant=None):
    """out[v] = x[row_start[v]] for the V = row_start.numel() - 1 voxels of a row level; variant "f16" / "bf16": cast to that
    build's 16-bit type, saturating."""
    _need_gpu(x, row_start)
    nv = row_start.numel() - 1
    out = torch.empty((nv, x.shape[1]), dtype=torch.float32 if variant is None else LP_DTYPES[variant], device=x.device)
    check(_lib.load(variant).cdseg_gather_first(_ptr(x), _ptr(row_start), _ptr(out), F32 if variant is None else BF16, nv, x.shape[1],
                                                _stream()), "gather_first")
    return out


def residual_rows(x, a, row_vox, t_rows=None, scene_offs=None, out=None):
    """out = x + a[row_vox] + t_rows[scene(row)] (fp32, adds rounded separately: bit-equal to torch)."""
    _need_gpu(x, a, row_vox)
    out = torch.empty_like(x) if out is None else out
    check(_lib.load().cdseg_residual_rows(_ptr(x), _ptr(a), _ptr(row_vox), _ptr(t_rows), _ptr(scene_offs),
                                          0 if t_rows is None else t_rows.shape[0], _ptr(out), x.shape[0], x.shape[1], _stream()),
          "residual_rows")
    return out


def run_sum(dx, row_start):
    """out[v] = sum of the rows row_start[v] .. row_start[v + 1] - 1 of dx, ascending (fp32)."""
    _need_gpu(dx, row_start)
    nv = row_start.numel() - 1
    out = torch.empty((nv, dx.shape[1]), dtype=torch.float32, device=dx.device)
    check(_lib.load().cdseg_run_sum(_ptr(dx), _ptr(row_start), _ptr(out), nv, dx.shape[1], _stream()), "run_sum")
    return out


def scatter_first(g, row_vox, row_start, dx=None):
    """The conv's data gradient g (one row per voxel) on the first row of every run: added into dx when given, else a new
    (n, c) tensor whose other rows are zero."""
    _need_gpu(g, row_vox, row_start)
    acc = dx is not None
    if not acc:
        dx = torch.empty((row_vox.numel(), g.shape[1]), dtype=torch.float32, device=g.device)
    check(_lib.load().cdseg_scatter_first(_ptr(g), _ptr(row_vox), _ptr(row_start), _ptr(dx), int(acc), dx.shape[0], g.shape[1],
                                          _stream()), "scatter_first")
    return dx


def _row_out(like, lp_variant):
    return torch.empty(like.shape, dtype=torch.float32 if lp_variant is None else LP_DTYPES[lp_variant], device=like.device)


def residual(x, a=None, mask=None, t_rows=None, scene_offs=None, out=None):
    """out = x + mask[row] * a + t_rows[scene(row)] (fp32; multiply and add rounded separately: bit-equal to torch)."""
    _need_gpu(x)
    out = torch.empty_like(x) if out is None else out
    check(_lib.load().cdseg_residual(_ptr(x), _ptr(a), _ptr(mask), _ptr(t_rows), _ptr(scene_offs),
                                     0 if t_rows is None else t_rows.shape[0], _ptr(out), x.shape[0], x.shape[1], _stream()), "residual")
    return out


def scale_cast(dy, mask=None, variant=None):
    """cast(mask[row] * dy) WITHOUT saturation: fp32 (variant None) or the 16-bit type of build `variant` (torch's `.to`)."""
    _need_gpu(dy)
    out = _row_out(dy, variant)
    check(_lib.load(variant).cdseg_scale_cast(_ptr(dy), _ptr(mask), _ptr(out), dt(out) if variant is None else BF16, dy.shape[0],
                                              dy.shape[1], _stream()), "scale_cast")
    return out


def add_layernorm(x, a, mask, gamma, beta, eps=1e-5, variant=None):
    """(x1, h): x1 = x + mask[row] * a, h = LayerNorm(x1) in fp32 or the 16-bit type of build `variant`; one pass."""
    _need_gpu(x, a)
    x1, h = torch.empty_like(x), _row_out(x, variant)
    check(_lib.load(variant).cdseg_add_layernorm(_ptr(x), _ptr(a), _ptr(mask), _ptr(gamma), _ptr(beta), float(eps), _ptr(x1), _ptr(h),
                                                 F32 if variant is None else BF16, x.shape[0], x.shape[1], _stream()), "add_layernorm")
    return x1, h


def gelu_fwd(u, variant=None):
    """GELU(u) (erf form) in fp32 or the 16-bit type of build `variant`."""
    _need_gpu(u)
    g = _row_out(u, variant)
    check(_lib.load(variant).cdseg_gelu_fwd(_ptr(u), _ptr(g), F32 if variant is None else BF16, u.numel(), _stream()), "gelu_fwd")
    return g


def gelu_bwd_cast(u, dg, variant=None):
    """dg * GELU'(u) in fp32 or, without saturation, the 16-bit type of build `variant`."""
    _need_gpu(u, dg)
    du = _row_out(u, variant)
    check(_lib.load(variant).cdseg_gelu_bwd_cast(_ptr(u), _ptr(dg), _ptr(du), F32 if variant is None else BF16, u.numel(), _stream()),
          "gelu_bwd_cast")
    return du


# ------------------------------------------------------------------ train-mode BatchNorm + GELU, pooling maximum (csrc/norm.hip)
BN_WIDTHS = range(16, 513, 16)  # channel counts of the kernels of csrc/norm.hip


class RowPartition(tuple):
    """(rows_per_block, blocks) of a fixed-order column sum (csrc/colsum.h: the two BatchNorm reduction passes, the skip
    statistics): block b covers rows b * rows_per_block .. (the last may be shorter); the order in which the block partials are
    added is the op's (BatchNorm: ascending block index; skip statistics: 16 segments of consecutive blocks)."""
    __slots__ = ()
    rows_per_block = property(lambda self: self[0])
    blocks = property(lambda self: self[1])


def _sums_ws(ws_bytes, rows, c, device):
    """The block partials of a fixed-order column sum, sized by the op's cdseg_*_ws_bytes (never empty: the pointer is checked)."""
    return _scratch(max(16, ws_bytes(int(rows), int(c))), device)


def bn_partition(m, c):
    """Row partition of `bn_stats` and of the sums of `bn_gelu_bwd` for an (m, c) input: a function of the shape only (host
    code, no GPU needed, the same in both builds)."""
    rows, blocks = ctypes.c_long(0), ctypes.c_int(0)
    check(_lib.load().cdseg_bn_partition(int(m), int(c), ctypes.byref(rows), ctypes.byref(blocks)), "bn_partition")
    return RowPartition((rows.value, blocks.value))


def _bn_rows(what, *ts):
    """fp32 (rows, c) operands with contiguous rows (any row stride: column slices of wider buffers pass)."""
    for t in ts:
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.shape != ts[0].shape:
            raise _lib.CdsegError(f"{what}: fp32 (rows, c) tensors of one shape with contiguous rows")


def _a16(t):
    """A per-channel vector the kernels load 16 bytes at a time: contiguous fp32, 16-byte aligned (a copy only if it is not)."""
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def bn_stats(x):
    """Per-channel statistics of fp32 x (m, c): a (2 c + 1) fp64 device tensor [sum x, sum x^2, m], summed in fp64 in an order
    fixed by (m, c) (cdseg_bn_stats).  Buffers of several row shards merge by plain addition; m = 0 gives zeros."""
    _need_gpu(x)
    _bn_rows("bn_stats", x)
    m, c = x.shape
    if m == 0:
        return torch.zeros(2 * c + 1, dtype=torch.float64, device=x.device)
    lib = _lib.load()
    stats = torch.empty(2 * c + 1, dtype=torch.float64, device=x.device)
    ws = _sums_ws(lib.cdseg_bn_ws_bytes, m, c, x.device)
    check(lib.cdseg_bn_stats(_ptr(x), x.stride(0), m, c, _ptr(stats), _ptr(ws), ws.numel(), _stream()), "bn_stats")
    return stats


def bn_finish(stats, eps, momentum, running_mean=None, running_var=None):
    """(mean, invstd) fp32 (c) from a (merged) statistics buffer; the row count is read from stats[2 c] on the device.
    running_mean / running_var (fp32, contiguous) are updated in place like nn.BatchNorm1d (unbiased variance)."""
    _need_gpu(stats)
    c = (stats.numel() - 1) // 2
    assert stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() == 2 * c + 1
    for r in (running_mean, running_var):
        assert r is None or (r.dtype == torch.float32 and r.is_contiguous() and r.numel() == c)
    mean = torch.empty(c, dtype=torch.float32, device=stats.device)
    invstd = torch.empty(c, dtype=torch.float32, device=stats.device)
    check(_lib.load().cdseg_bn_finish(_ptr(stats), c, float(eps), float(momentum), _ptr(mean), _ptr(invstd), _ptr(running_mean),
                                      _ptr(running_var), _stream()), "bn_finish")
    return mean, invstd


def bn_gelu_fwd(x, mean, invstd, gamma, beta, out=None):
    """y = GELU(gamma (x - mean) invstd + beta), erf form (cdseg_bn_gelu_fwd); out: a (m, c) fp32 view to write into."""
    _need_gpu(x)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device) if out is None else out
    _bn_rows("bn_gelu_fwd", x, y)
    m, c = x.shape
    check(_lib.load().cdseg_bn_gelu_fwd(_ptr(x), x.stride(0), m, c, _ptr(_a16(mean)), _ptr(_a16(invstd)), _ptr(_a16(gamma)),
                                        _ptr(_a16(beta)), _ptr(y), y.stride(0), _stream()), "bn_gelu_fwd")
    return y


def bn_gelu_bwd(x, dy, mean, invstd, gamma, beta, count, hook=None, out=None):
    """Backward of `bn_gelu_fwd` over batch statistics: returns (dx, gsums) with gsums (2 c) fp64 = [sum g, sum g x_hat] over
    THESE rows (dbeta, dgamma), g = dy GELU'(z) recomputed from x.  count: fp64 device tensor whose first element is the row
    count behind mean / invstd (a view of the statistics buffer).  hook(gsums) -> the sums dx is formed with (SyncBN: the sums
    over all ranks); it runs between the two passes, also for m = 0.  out: a (m, c) fp32 view for dx."""
    _need_gpu(x, dy, count)
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device) if out is None else out
    _bn_rows("bn_gelu_bwd", x, dy, dx)
    assert count.dtype == torch.float64 and count.numel() >= 1
    m, c = x.shape
    lib = _lib.load()
    mean, invstd, gamma, beta = _a16(mean), _a16(invstd), _a16(gamma), _a16(beta)
    if m == 0:
        gsums = torch.zeros(2 * c, dtype=torch.float64, device=x.device)
    else:
        gsums = torch.empty(2 * c, dtype=torch.float64, device=x.device)
        ws = _sums_ws(lib.cdseg_bn_ws_bytes, m, c, x.device)
        check(lib.cdseg_bn_gelu_bwd_sums(_ptr(x), x.stride(0), _ptr(dy), dy.stride(0), m, c, _ptr(mean), _ptr(invstd), _ptr(gamma),
                                         _ptr(beta), _ptr(gsums), _ptr(ws), ws.numel(), _stream()), "bn_gelu_bwd (sums)")
    total = gsums if hook is None else hook(gsums).contiguous()
    check(lib.cdseg_bn_gelu_bwd_dx(_ptr(x), x.stride(0), _ptr(dy), dy.stride(0), m, c, _ptr(mean), _ptr(invstd), _ptr(gamma),
                                   _ptr(beta), _ptr(total), _ptr(count), _ptr(dx), dx.stride(0), _stream()), "bn_gelu_bwd (dx)")
    return dx, gsums


def _fg_rows(what, *ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.shape != ts[0].shape):
            raise _lib.CdsegError(f"{what}: contiguous fp32 (rows, c) tensors of one shape")


def _fg_mask(what, m, rows):
    if m is None:
        return None
    if m.dtype != torch.float32 or not m.is_contiguous() or m.numel() != rows:
        raise _lib.CdsegError(f"{what}: the DropPath factors are one contiguous fp32 value per row")
    return m


def fuse_gate_fwd(s, a, alpha, gamma, m=None, out=None):
    """The fusion gate of a CrossBlock (cdseg_fuse_gate_fwd): y = alpha * s + gamma * m[:, None] * a on fp32 (rows, c); alpha,
    gamma (c) per channel, m (rows) the DropPath factors or None; a None: y = alpha * s.  out: the tensor to write (may be s).
    c up to 512; a width that is no multiple of 4, or an operand off a 16-byte boundary, takes the library's scalar path."""
    _need_gpu(s, a, m, alpha, gamma)
    y = torch.empty_like(s) if out is None else out
    _fg_rows("fuse_gate_fwd", s, a, y)
    rows, c = s.shape
    check(_lib.load().cdseg_fuse_gate_fwd(_ptr(s), _ptr(a), _ptr(_fg_mask("fuse_gate_fwd", m, rows)), _ptr(_a16(alpha)),
                                          _ptr(_a16(gamma)), _ptr(y), rows, c, _stream()), "fuse_gate_fwd")
    return y


def fuse_gate_bwd(dy, s, a, alpha, gamma, m=None):
    """Backward of `fuse_gate_fwd` (cdseg_fuse_gate_bwd): returns (ds, da, sums) with ds = alpha * dy, da = gamma * m * dy and
    sums (2 c) fp64 = [sum_r dy m a, sum_r dy s] - the gradients of gamma and of alpha - added in fp64 in an order fixed by the
    shape (no atomics: equal inputs give equal bits)."""
    _need_gpu(dy, s, a, m, alpha, gamma)
    _fg_rows("fuse_gate_bwd", dy, s, a)
    rows, c = s.shape
    ds, da = torch.empty_like(s), torch.empty_like(s)
    if rows == 0:
        return ds, da, torch.zeros(2 * c, dtype=torch.float64, device=s.device)
    lib = _lib.load()
    sums = torch.empty(2 * c, dtype=torch.float64, device=s.device)
    ws = _sums_ws(lib.cdseg_fuse_gate_ws_bytes, rows, c, s.device)
    check(lib.cdseg_fuse_gate_bwd(_ptr(dy), _ptr(s), _ptr(a), _ptr(_fg_mask("fuse_gate_bwd", m, rows)), _ptr(_a16(alpha)),
                                  _ptr(_a16(gamma)), _ptr(ds), _ptr(da), _ptr(sums), rows, c, _ptr(ws), ws.numel(), _stream()),
          "fuse_gate_bwd")
    return ds, da, sums


def _sk_rows(what, t, dtypes):
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype not in dtypes:
        raise _lib.CdsegError(f"{what}: a (rows, c) tensor with unit column stride, dtype one of {dtypes}")


def _sk_map(what, m, n):
    if m is not None and (m.dtype != torch.int32 or not m.is_contiguous() or m.numel() != n):
        raise _lib.CdsegError(f"{what}: the row map is one contiguous int32 value per row")
    return m


def skip_partition(n, c):
    """(rows_per_chunk, chunks) of `skip_stats` for an (n, c) feature: host only, a function of the shape."""
    rpc, chunks = ctypes.c_long(0), ctypes.c_int(0)
    check(_lib.load().cdseg_skip_partition(int(n), int(c), ctypes.byref(rpc), ctypes.byref(chunks)), "skip_partition")
    return RowPartition((rpc.value, chunks.value))


def skip_stats(x, ref_of_row=None, n_total=None):
    """[S0 A B] (3 c) fp64 of the skip feature x (n, c), fp32 or the active build's 16-bit type (cdseg_skip_stats): the three
    column sums behind FreeU's Fourier filter, with cos / sin of 2 pi m / n_total at the REFERENCE row m = ref_of_row[r]
    (int32, physical row -> reference row; None = identity).  fp64 sums in an order fixed by the shape: equal inputs give
    equal bits.  No host read."""
    _need_gpu(x, ref_of_row)
    _sk_rows("skip_stats", x, (torch.float32, LP_DTYPES[_lib.active()]))
    n, c = x.shape
    n_total = n if n_total is None else int(n_total)
    if n == 0:
        return torch.zeros(3 * c, dtype=torch.float64, device=x.device)
    lib = _lib.load()
    stats = torch.empty(3 * c, dtype=torch.float64, device=x.device)
    ws = _sums_ws(lib.cdseg_skip_stats_ws_bytes, n, c, x.device)
    check(lib.cdseg_skip_stats(_ptr(x), dt(x), x.stride(0), n, c, _ptr(_sk_map("skip_stats", ref_of_row, n)), n_total, _ptr(stats),
                               _ptr(ws), ws.numel(), _stream()), "skip_stats")
    return stats


def skip_fold(w, stats):
    """u (3 cout) fp64 = [W S0, W A, W B] for the (cout, cin) matrix w (fp32 or the 16-bit type) and `skip_stats`' output:
    what the filter adds behind a Linear that reads the filtered feature (cdseg_skip_fold)."""
    _need_gpu(w, stats)
    _sk_rows("skip_fold", w, (torch.float32, LP_DTYPES[_lib.active()]))
    cout, cin = w.shape
    assert stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() == 3 * cin
    u = torch.empty(3 * cout, dtype=torch.float64, device=w.device)
    check(_lib.load().cdseg_skip_fold(_ptr(w), dt(w), w.stride(0), cout, cin, _ptr(stats), _ptr(u), _stream()), "skip_fold")
    return u


def skip_merge(x, stats=None, s=1.0, f=1.0, ref_of_row=None, n_total=None, child=None, cluster=None, folded=False):
    """In place on the fp32 stream x (n, c) (cdseg_skip_merge), k = (float32(s) - 1) / n_total:
        x = f * (x + k * (S0 + A cos t_r + B sin t_r)) + child[cluster]
        folded (stats = `skip_fold`'s u, x carries f already):  x = x + f * k * (u0 + u1 cos t_r + u2 sin t_r) + child[cluster]
    stats None: f * x + child[cluster]; child None: the scaled / filtered skip alone.  Returns x."""
    _need_gpu(x, stats, ref_of_row, child, cluster)
    _sk_rows("skip_merge", x, (torch.float32,))
    n, c = x.shape
    n_total = n if n_total is None else int(n_total)
    if stats is not None:
        assert stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() == 3 * c
    if child is not None:
        _sk_rows("skip_merge", child, (torch.float32,))
        assert child.shape[1] == c and cluster is not None
        _sk_map("skip_merge", cluster, n)
    check(_lib.load().cdseg_skip_merge(_ptr(x), x.stride(0), n, c, _ptr(stats), int(bool(folded)), float(s), n_total, float(f),
                                       _ptr(_sk_map("skip_merge", ref_of_row, n)), _ptr(child),
                                       0 if child is None else child.stride(0), _ptr(cluster),
                                       0 if child is None else child.shape[0], _stream()), "skip_merge")
    return x


def segment_max_arg(y, seg_start, m):
    """(out, arg): out (m, c) fp32 = per-channel maximum over the rows seg_start[j] .. seg_start[j + 1] - 1 of y (the bits of
    `segment_max` without scale / shift / activation), arg (m, c) int32 = the first row that holds it (cdseg_segment_max_arg)."""
    _need_gpu(y, seg_start)
    _bn_rows("segment_max_arg", y)
    assert seg_start.dtype == torch.int32 and seg_start.numel() >= m + 1
    c = y.shape[1]
    out = torch.empty((m, c), dtype=torch.float32, device=y.device)
    arg = torch.empty((m, c), dtype=torch.int32, device=y.device)
    check(_lib.load().cdseg_segment_max_arg(_ptr(y), y.stride(0), _ptr(seg_start), int(m), c, _ptr(out), out.stride(0), _ptr(arg),
                                            arg.stride(0), _stream()), "segment_max_arg")
    return out, arg


def segment_max_bwd(dout, arg, cluster):
    """dy (n, c) fp32: dy[i] = dout[cluster[i]] where arg[cluster[i]] == i, else 0, per channel; one launch that writes every
    element once (cdseg_segment_max_bwd).  cluster (n) int32: the pooled row of every fine row."""
    _need_gpu(dout, arg, cluster)
    _bn_rows("segment_max_bwd", dout)
    assert arg.dtype == torch.int32 and arg.shape == dout.shape and arg.stride(1) == 1
    assert cluster.dtype == torch.int32 and cluster.is_contiguous()
    n, c = cluster.numel(), dout.shape[1]
    dy = torch.empty((n, c), dtype=torch.float32, device=dout.device)
    check(_lib.load().cdseg_segment_max_bwd(_ptr(dout), dout.stride(0), _ptr(arg), arg.stride(0), _ptr(cluster), n, c, _ptr(dy),
                                            dy.stride(0), _stream()), "segment_max_bwd")
    return dy


# ------------------------------------------------------------------ fused segmentation loss (csrc/loss.hip)
def seg_loss_plan(logits, labels, ignore_index):
    """The fused loss's ONE host read: the label histogram of the valid rows (cdseg_seg_loss_fwd phase 0).  Returns the plan
    `seg_loss` needs - dict(labels, ignore_index, hist_host, n_valid, present) - or None for a batch without a valid row (no
    fused form: the caller's torch path produces the reference's nan / 0).  Labels outside [0, C) other than ignore_index raise."""
    _need_gpu(logits, labels)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise _lib.CdsegError("seg_loss: logits must be fp32 (N, C) with contiguous rows")
    n, c = logits.shape
    if labels.dtype != torch.int64 or labels.shape != (n,):
        raise _lib.CdsegError("seg_loss: labels must be int64 (N)")
    labels = labels.contiguous()
    ign = int(ignore_index)
    hist = torch.empty(c + 1, dtype=torch.int32, device=logits.device)
    check(_lib.load().cdseg_seg_loss_fwd(_ptr(logits), logits.stride(0), _ptr(labels), n, c, ign, 0, _ptr(hist), None, None, None,
                                         None, 0, _stream()), "seg_loss (histogram)")
    hist_list = hist.tolist()  # the one host read
    if hist_list[c]:
        raise _lib.CdsegError(f"seg_loss: {hist_list[c]} labels outside [0, {c}) that are not ignore_index = {ign}")
    n_valid, present = sum(hist_list[:c]), sum(1 for v in hist_list[:c] if v)
    if n_valid == 0:
        return None
    return dict(labels=labels, ignore_index=ign, hist_host=(ctypes.c_int32 * (c + 1))(*hist_list), n_valid=n_valid, present=present)


def seg_loss(logits, labels, ignore_index, plan=None):
    """Cross entropy + multi-class Lovasz-Softmax (classes present, whole batch) of fp32 logits (N, C; any row stride) and int64
    labels in a handful of launches (cdseg_seg_loss_fwd; definition and tie rule - descending error, ascending row index - in
    include/cdseg.h).  Returns (ce, lovasz, saved): two 0-dim fp32 tensors and what `seg_loss_bwd` needs (the plan + coef).
    plan: from `seg_loss_plan` on the same tensors (made here when None); a batch without a valid row gives (None, None, None)."""
    if plan is None:
        plan = seg_loss_plan(logits, labels, ignore_index)
        if plan is None:
            return None, None, None
    _need_gpu(logits)
    n, c = logits.shape
    lib = _lib.load()
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    coef = torch.empty((n, plan["present"]), dtype=torch.float32, device=logits.device)
    ws = _scratch(max(16, lib.cdseg_seg_loss_ws_bytes(n, c)), logits.device)
    check(lib.cdseg_seg_loss_fwd(_ptr(logits), logits.stride(0), _ptr(plan["labels"]), n, c, plan["ignore_index"], 1, None,
                                 plan["hist_host"], _ptr(out), _ptr(coef), _ptr(ws), ws.numel(), _stream()), "seg_loss")
    return out[0], out[1], dict(plan, coef=coef)


def seg_loss_bwd(logits, saved, g_ce, g_lovasz):
    """dlogits (N, C) fp32 = g_ce * dCE/dlogits + g_lovasz * dLovasz/dlogits in one launch (cdseg_seg_loss_bwd); g_* are 0-dim
    fp32 device tensors or None (= 0); `saved` from `seg_loss` on the same logits."""
    _need_gpu(logits)
    n, c = logits.shape
    gs = []
    for g in (g_ce, g_lovasz):
        if g is not None:
            _need_gpu(g)
            g = g.reshape(1).to(torch.float32).contiguous()
        gs.append(g)
    dlogits = torch.empty((n, c), dtype=torch.float32, device=logits.device)
    check(_lib.load().cdseg_seg_loss_bwd(_ptr(logits), logits.stride(0), _ptr(saved["labels"]), n, c, saved["ignore_index"],
                                         saved["hist_host"], _ptr(saved["coef"]), _ptr(gs[0]), _ptr(gs[1]), _ptr(dlogits),
                                         dlogits.stride(0), _stream()), "seg_loss_bwd")
    return dlogits


# ------------------------------------------------------------------ train-time pipeline ops (csrc/traintime.hip)
TT_CENTER_NONE, TT_CENTER_HOST, TT_CENTER_BBOX, TT_CENTER_SHIFT_Z, TT_CENTER_SHIFT_XY = 0, 1, 2, 3, 4  # include/cdseg.h


def _d3(v, n=3):
    return None if v is None else (ctypes.c_double * n)(*[float(x) for x in v])


def tt_bbox(xyz):
    """(6,) float64 on the device: [min x y z, max x y z] of an (n,3) float32 / float64 array (n >= 1)."""
    _need_gpu(xyz)
    assert xyz.dtype in (torch.float32, torch.float64) and xyz.dim() == 2 and xyz.shape[1] == 3 and xyz.shape[0] > 0
    xyz = xyz.contiguous()
    ws = torch.empty(12, dtype=torch.float64, device=xyz.device)
    check(_lib.load().cdseg_tt_bbox(_ptr(xyz), 1 if xyz.dtype == torch.float64 else 0, xyz.shape[0], _ptr(ws), _stream()),
          "tt_bbox")
    return ws[6:]


def tt_affine(xyz, center=TT_CENTER_NONE, center3=None, bbox=None, rot=None, add_back=False, scale=None, flipx=False,
              flipy=False, out_dtype=torch.float64):
    """((xyz - c) R^T [+ c]) [* scale], flips: one pass in float64 without fused multiply-adds (include/cdseg.h).
    xyz (n,3) float32 / float64; rot: 3x3 nested floats or None; -> a new (n,3) tensor of out_dtype."""
    _need_gpu(xyz, bbox)
    assert xyz.dtype in (torch.float32, torch.float64) and out_dtype in (torch.float32, torch.float64)
    xyz = xyz.contiguous()
    n = xyz.shape[0]
    out = torch.empty((n, 3), dtype=out_dtype, device=xyz.device)
    r = None if rot is None else (ctypes.c_double * 9)(*[float(v) for row in rot for v in row])
    check(_lib.load().cdseg_tt_affine(_ptr(xyz), 1 if xyz.dtype == torch.float64 else 0, n, int(center), _d3(center3), _ptr(bbox),
                                      r, 1 if add_back else 0, float(scale if scale is not None else 1.0),
                                      1 if scale is not None else 0, 1 if flipx else 0, 1 if flipy else 0, _ptr(out),
                                      1 if out_dtype == torch.float64 else 0, _stream()), "tt_affine")
    return out


def tt_jitter(coord, z, sigma, clip):
    """coord (n,3) float64 += clip(sigma * z), in place; z (n,3) float32 or float64."""
    _need_gpu(coord, z)
    assert coord.dtype == torch.float64 and coord.is_contiguous() and z.dtype in (torch.float32, torch.float64)
    z = z.contiguous()
    assert z.numel() == coord.numel()
    check(_lib.load().cdseg_tt_jitter(_ptr(coord), _ptr(z), 1 if z.dtype == torch.float64 else 0, float(sigma), float(clip),
                                      coord.shape[0], _stream()), "tt_jitter")
    return coord


def tt_blur(noise):
    """The reference's smoothing of an elastic noise grid (d0,d1,d2,3) float32: box filter along x, y, z, twice."""
    _need_gpu(noise)
    assert noise.dtype == torch.float32 and noise.dim() == 4 and noise.shape[3] == 3
    src, bufs = noise.contiguous(), (torch.empty_like(noise), torch.empty_like(noise))  # the input grid is left as it is
    d0, d1, d2 = (int(v) for v in noise.shape[:3])
    lib = _lib.load()
    for k in range(6):
        dst = bufs[k & 1]
        check(lib.cdseg_tt_blur3(_ptr(src), d0, d1, d2, k % 3, _ptr(dst), _stream()), "tt_blur3")
        src = dst
    return src


def tt_elastic(coord, noise, start, step, stop, magnitude):
    """coord (n,3) float64 += trilinear(noise)(coord) * magnitude, in place; noise (d0,d1,d2,3) float32 (blurred)."""
    _need_gpu(coord, noise)
    assert coord.dtype == torch.float64 and coord.is_contiguous() and noise.dtype == torch.float32 and noise.is_contiguous()
    dims = (ctypes.c_int * 3)(*[int(v) for v in noise.shape[:3]])
    check(_lib.load().cdseg_tt_elastic(_ptr(coord), coord.shape[0], _ptr(noise), dims, _d3(start), _d3(step), _d3(stop),
                                       float(magnitude), _stream()), "tt_elastic")
    return coord


def tt_color(color, bbox=None, blend=None, tr=None, noise=None, noise_mul=0.0):
    """The colour chain on (n,3) float32 in place: auto contrast (bbox, blend), translation (tr), jitter (noise)."""
    _need_gpu(color, bbox, noise)
    assert color.dtype == torch.float32 and color.is_contiguous()
    if noise is not None:
        assert noise.dtype in (torch.float32, torch.float64) and noise.numel() == color.numel()
        noise = noise.contiguous()
    check(_lib.load().cdseg_tt_color(_ptr(color), color.shape[0], _ptr(bbox), float(blend if blend is not None else 0.0),
                                     1 if blend is not None else 0, _d3(tr), _ptr(noise),
                                     1 if (noise is not None and noise.dtype == torch.float64) else 0, float(noise_mul),
                                     _stream()), "tt_color")
    return color


def tt_voxel_pick(idx_sort, seg_start, m, r):
    """Raw row of member r[v] % count[v] of every voxel v; r (m,) int64 >= 0."""
    _need_gpu(idx_sort, seg_start, r)
    assert r.dtype == torch.int64 and r.numel() >= int(m)
    out = torch.empty(int(m), dtype=torch.int32, device=idx_sort.device)
    check(_lib.load().cdseg_tt_voxel_pick(_ptr(idx_sort), _ptr(seg_start), int(m), _ptr(r.contiguous()), _ptr(out), _stream()),
          "tt_voxel_pick")
    return out


def tt_dist_key(coord, center):
    """Sort keys (n,) int64 of the float64 squared distances of coord (n,3) float64 to its row `center`."""
    _need_gpu(coord)
    assert coord.dtype == torch.float64 and coord.is_contiguous()
    key = torch.empty(coord.shape[0], dtype=torch.int64, device=coord.device)
    check(_lib.load().cdseg_tt_dist_key(_ptr(coord), coord.shape[0], int(center), _ptr(key), _stream()), "tt_dist_key")
    return key


def rand_int(n, seed, offset, device, bound=0, bound_dev=None):
    """n Philox integers (int64): raw 32-bit words, or reduced modulo `bound` / the device int32 `bound_dev`."""
    out = torch.empty(int(n), dtype=torch.int64, device=device)
    check(_lib.load().cdseg_rand_int(_ptr(out), int(n), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), _ptr(bound_dev),
                                     int(bound), _stream()), "rand_int")
    return out
