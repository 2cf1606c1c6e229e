"""Row-block sharding of one raster across the ranks of a node.

One process per GPU (`torch.distributed`; backend "nccl" is RCCL over xGMI on
ROCm, "gloo" on CPU for tests).  Shard g of G owns rows [g*R/G, (g+1)*R/G) of the
row-major raster (ec_shard_range); operands, masks and outputs use the same
split, so every element-wise kernel is local and needs no communication.  The
only exchanges are reductions of scalars:

  min_max  each rank reduces its shard to two order-preserving int64 keys
           {~key(min), key(max)} on its own GPU (ec_min_max_keys); one
           all_reduce(MAX) of that 16-byte tensor; decode (ec_min_max_decode).
  counts   all_reduce(SUM) of {n_true, n_false}.

The collective is latency-bound (16 B); link bandwidth is irrelevant.
"""
from __future__ import annotations

import ctypes as C

from . import buffer as B
from ._ffi import EcStats, EcValue, check, lib


def shard_range(n_rows: int, n_cols: int, shard: int, n_shards: int) -> tuple[int, int]:
    """(cell_offset, cell_len) of a row-block shard."""
    off, ln = C.c_uint64(), C.c_uint64()
    check(lib().ec_shard_range(n_rows, n_cols, shard, n_shards, C.byref(off), C.byref(ln)))
    return off.value, ln.value


def combine_min_max_keys(ct: int, keys2) -> tuple[B.CellValue, B.CellValue]:
    """Decode all-reduced {~key(min), key(max)} into typed values."""
    arr = (C.c_int64 * 2)(int(keys2[0]), int(keys2[1]))
    mn, mx = EcValue(), EcValue()
    check(lib().ec_min_max_decode(ct, arr, C.byref(mn), C.byref(mx)))
    return B.CellValue.from_ec(mn), B.CellValue.from_ec(mx)


def sharded_min_max(local, group=None):
    """Global (min, max) of a raster whose local row-block is `local`
    (CellBuffer or MaskedCellBuffer on this rank's GPU).  Collective."""
    import torch
    import torch.distributed as dist

    buf = local.buffer() if isinstance(local, B.MaskedCellBuffer) else local
    mask_ptr = local.mask().mem.ptr if isinstance(local, B.MaskedCellBuffer) else None
    keys = torch.empty(2, dtype=torch.int64, device="cuda")
    B.set_stream(torch.cuda.current_stream().cuda_stream)  # same stream RCCL will order after
    check(lib().ec_min_max_keys(buf.ct, buf.mem.ptr, mask_ptr, buf.n, keys.data_ptr(), B.stream()))
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(keys, op=dist.ReduceOp.MAX, group=group)
    k = keys.cpu()
    return combine_min_max_keys(buf.ct, (int(k[0]), int(k[1])))


def sharded_counts(local_mask: B.Mask, group=None) -> tuple[int, int]:
    """Global (data, nodata) counts of a row-sharded mask.  Collective."""
    import torch
    import torch.distributed as dist

    counts = torch.empty(2, dtype=torch.int64, device="cuda")
    B.set_stream(torch.cuda.current_stream().cuda_stream)
    check(lib().ec_mask_counts_device(local_mask.mem.ptr, local_mask.n, counts.data_ptr(), B.stream()))
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=group)
    c = counts.cpu()
    return int(c[0]), int(c[1])


def allreduce_keys_host(keys2, group=None):
    """The same key exchange on host tensors (gloo): used by the CPU multi-process tests."""
    import torch
    import torch.distributed as dist

    t = torch.tensor([int(keys2[0]), int(keys2[1])], dtype=torch.int64)
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return int(t[0]), int(t[1])


# --------------------------------------------------------------------------- one process, all GPUs
class ShardedBuffer:
    """A raster cut into row-blocks, block i in device i's HBM (cells of one type, or a mask with ct = UInt8)."""

    def __init__(self, group: "ShardGroup", ct: int, ptrs, lens):
        self.group, self.ct, self.ptrs, self.lens = group, ct, ptrs, list(lens)

    def len(self) -> int:
        return sum(self.lens)

    def free(self) -> None:
        if self.ptrs is not None:
            check(lib().ec_sharded_free(self.group.handle, self.ptrs))
            self.ptrs = None


class ShardGroup:
    """`ec_shard_group`: one process driving the listed GPUs — per device a launch thread, a stream and a communicator
    of the clique inside the library.  `host_combine=True` folds the 16-byte reduction payloads on the host instead of
    over xGMI (no RCCL; lets one device be listed several times, e.g. to rehearse on a 1-GPU box)."""

    def __init__(self, devices, host_combine: bool = False, blocking_issue: bool = False):
        """`blocking_issue=True`: every element-wise call waits until all launch threads have issued (the form of rounds
        1-2); default: the calls are queued for the launch threads and return at once, a failure inside one is raised by
        the next `sync()` / reduction."""
        self.n = len(devices)
        self.handle = C.c_void_p()
        arr = (C.c_int32 * self.n)(*devices)
        flags = (1 if host_combine else 0) | (2 if blocking_issue else 0)
        check(lib().ec_shard_group_create(arr, self.n, flags, C.byref(self.handle)))

    def close(self) -> None:
        if self.handle:
            for tabs in getattr(self, "_owned_tables", []):   # the reclass tables replicated by reclassify()
                tabs.free()
            self._owned_tables = []
            check(lib().ec_shard_group_destroy(self.handle))
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def shard(self, i: int):
        dev, st = C.c_int32(), C.c_void_p()
        check(lib().ec_shard_group_shard(self.handle, i, C.byref(dev), C.byref(st)))
        return dev.value, st.value

    def sync(self) -> None:
        """Everything queued so far has been issued and has finished; raises the first failure a queued call left behind."""
        check(lib().ec_shard_group_sync(self.handle))

    def stat(self, key: str) -> int:
        v = C.c_int64()
        check(lib().ec_shard_group_stat(self.handle, key.encode(), C.byref(v)))
        return v.value

    def foreach(self, fn) -> None:
        """fn(shard, device, stream) on every shard's own launch thread (its device current); any ABI call may be made
        there on `stream`.  An exception raised by fn is re-raised here."""
        from ._ffi import SHARD_FN, EC_ERR_ARG
        raised = []

        def tramp(shard, device, stream, _user):
            try:
                fn(shard, device, stream)
                return 0
            except Exception as e:  # noqa: BLE001 — carried across the C frame
                raised.append(e)
                return EC_ERR_ARG

        cb = SHARD_FN(tramp)
        st = lib().ec_shard_group_foreach(self.handle, cb, None)
        if raised:
            raise raised[0]
        check(st)

    def _sizes(self, lens, itemsize):
        return (C.c_size_t * self.n)(*[ln * itemsize for ln in lens])

    def alloc(self, ct: int, lens) -> ShardedBuffer:
        ptrs = (C.c_void_p * self.n)()
        check(lib().ec_sharded_alloc(self.handle, self._sizes(lens, B.NP_DTYPES[ct].itemsize), ptrs))
        return ShardedBuffer(self, ct, ptrs, lens)

    def scatter(self, a, n_rows: int, n_cols: int, ct: int = None) -> ShardedBuffer:
        """`From<Vec<T>>` of a row-major raster: contiguous row-blocks, block i to device i."""
        import numpy as np
        a = np.ascontiguousarray(a).ravel()
        assert a.size == n_rows * n_cols
        ct = B.cell_type_of(a.dtype) if ct is None else ct
        rng = [shard_range(n_rows, n_cols, g, self.n) for g in range(self.n)]
        out = self.alloc(ct, [r[1] for r in rng])
        sz = a.dtype.itemsize
        offs = (C.c_size_t * self.n)(*[r[0] * sz for r in rng])
        check(lib().ec_sharded_upload(self.handle, out.ptrs, a.ctypes.data_as(C.c_void_p), offs, self._sizes(out.lens, sz)))
        return out

    def gather(self, sb: ShardedBuffer):
        import numpy as np
        dt = B.NP_DTYPES[sb.ct]
        out = np.empty(sb.len(), dtype=dt)
        offs, acc = [], 0
        for ln in sb.lens:
            offs.append(acc * dt.itemsize)
            acc += ln
        check(lib().ec_sharded_download(self.handle, out.ctypes.data_as(C.c_void_p), sb.ptrs, (C.c_size_t * self.n)(*offs),
                                        self._sizes(sb.lens, dt.itemsize)))
        return out

    def binop(self, op: int, l: ShardedBuffer, r: ShardedBuffer) -> ShardedBuffer:
        assert l.lens == r.lens, "operands must be sharded identically"
        out = self.alloc(B.Float64, l.lens)
        check(lib().ec_sharded_binop(self.handle, op, l.ct, l.ptrs, r.ct, r.ptrs, (C.c_size_t * self.n)(*l.lens), out.ptrs))
        return out

    def compare(self, rel, l: ShardedBuffer, rhs, lmask: ShardedBuffer = None, rmask: ShardedBuffer = None) -> ShardedBuffer:
        """`CellBuffer.compare` on every shard, fire-and-forget: `rhs` an identically sharded buffer or a scalar; the sharded masks
        given are ANDed into the result.  Returns the sharded mask (ct = UInt8)."""
        r = B._relation(rel)
        lens = (C.c_size_t * self.n)(*l.lens)
        assert all(m is None or m.lens == l.lens for m in (lmask, rmask)), "masks must be sharded like their operand"
        out = self.alloc(B.UInt8, l.lens)
        lm = lmask.ptrs if lmask is not None else None
        if isinstance(rhs, ShardedBuffer):
            assert l.lens == rhs.lens, "operands must be sharded identically"
            check(lib().ec_sharded_compare(self.handle, r, l.ct, l.ptrs, lm, rhs.ct, rhs.ptrs, rmask.ptrs if rmask is not None else None,
                                           lens, out.ptrs))
        else:
            v = B.CellValue.new(rhs).to_ec()
            check(lib().ec_sharded_compare_scalar(self.handle, r, l.ct, l.ptrs, lm, lens, C.byref(v), out.ptrs))
        return out

    def cast(self, src: ShardedBuffer, ct: int, mode="round") -> ShardedBuffer:
        """`CellBuffer.cast` on every shard, fire-and-forget.  Returns the sharded buffer of type `ct`."""
        m = B._cast_mode(mode)
        out = self.alloc(ct, src.lens)
        check(lib().ec_sharded_cast(self.handle, m, src.ct, src.ptrs, ct, out.ptrs, (C.c_size_t * self.n)(*src.lens)))
        return out

    def to_scaled(self, src: ShardedBuffer, ct: int, scale: float, offset: float, mask: ShardedBuffer = None, no_data=None) -> ShardedBuffer:
        """`to_scaled` on every shard, fire-and-forget: `mask` (sharded like `src`) and the nodata scalar `no_data` together, or neither."""
        assert mask is None or mask.lens == src.lens, "the mask must be sharded like its operand"
        out = self.alloc(ct, src.lens)
        ev = B.CellValue(ct, no_data.value if isinstance(no_data, B.CellValue) else no_data).to_ec() if no_data is not None else None
        check(lib().ec_sharded_cast_scaled(self.handle, src.ct, src.ptrs, mask.ptrs if mask is not None else None, (C.c_size_t * self.n)(*src.lens),
                                           float(scale), float(offset), ct, C.byref(ev) if ev is not None else None, out.ptrs))
        return out

    def reclass_table(self, table: "B.ReclassTable") -> ShardedBuffer:
        """The table's record on every shard's device (ct = UInt8, EC_RECLASS_TABLE_BYTES each): replicate once, reuse across calls,
        `free()` it like any sharded buffer once the calls that use it have run."""
        from ._ffi import EC_RECLASS_TABLE_BYTES
        out = self.alloc(B.UInt8, [EC_RECLASS_TABLE_BYTES] * self.n)
        out.host = C.create_string_buffer(table.bytes(), EC_RECLASS_TABLE_BYTES)   # the source of the uploads: kept with the buffer
        check(lib().ec_sharded_upload(self.handle, out.ptrs, out.host, (C.c_size_t * self.n)(*[0] * self.n), self._sizes(out.lens, 1)))
        out.table = table
        return out

    def reclassify(self, src: ShardedBuffer, table_or_breaks, values=None, right: bool = False, dtype: int = None, valid=None,
                   mask: ShardedBuffer = None, nodata=None, breaks_dtype: int = None):
        """`reclassify` on every shard, fire-and-forget.  `table_or_breaks`: a replicated table (`reclass_table`), a ReclassTable or
        breaks with `values`; a table made here is replicated and freed by `close()`.  `mask` (sharded like `src`): the masked
        form, `nodata` (default 0) stored where it is 0.  Returns the sharded result — `(result, mask)` with a mask or a dropped class."""
        assert mask is None or mask.lens == src.lens, "the mask must be sharded like its operand"
        if isinstance(table_or_breaks, ShardedBuffer):
            tabs = table_or_breaks
            B._reclass_table(src.ct, tabs.table, values, right, dtype, valid, None if mask is None else 0, breaks_dtype)   # the checks
        else:
            nd = None if mask is None else (0 if nodata is None else nodata)
            tabs = self.reclass_table(B._reclass_table(src.ct, table_or_breaks, values, right, dtype, valid, nd, breaks_dtype))
            self._owned_tables = getattr(self, "_owned_tables", []) + [tabs]
        table = tabs.table
        out = self.alloc(table.dt, src.lens)
        om = self.alloc(B.UInt8, src.lens) if (mask is not None or table.drops) else None
        check(lib().ec_sharded_reclass(self.handle, src.ct, src.ptrs, mask.ptrs if mask is not None else None, (C.c_size_t * self.n)(*src.lens),
                                       table.dt, tabs.ptrs, out.ptrs, om.ptrs if om is not None else None))
        return (out, om) if om is not None else out

    def classify(self, src: ShardedBuffer, breaks, right: bool = False, mask: ShardedBuffer = None, breaks_dtype: int = None):
        """`classify` on every shard: a sharded UInt8 class raster with values 0 .. len(breaks), `(classes, mask)` with a mask."""
        import numpy as np
        return self.reclassify(src, breaks, np.arange(len(breaks) + 1, dtype=np.uint8), right=right, mask=mask,
                               nodata=None if mask is None else (255 if len(breaks) < 255 else 0), breaks_dtype=breaks_dtype)

    def _stack_call(self, what: str, layers, masks, min_count, aux: bool, result_type, call):
        """What `composite` and `composite_rank` do but for their own arguments: the stack's checks (texts start with `what`), the
        sharded result (cells of `result_type(cell type)`), its mask when a layer has one and the UInt8 aux buffer when asked for, and
        `call(cell type, layers, masks or None, K, n, dst, dst_mask or None, aux or None)`, which makes the library call."""
        from ._ffi import EC_COMPOSITE_MAX_LAYERS, EC_ERR_ARG, EcError, PVP
        layers = list(layers)
        k = len(layers)
        if not 1 <= k <= EC_COMPOSITE_MAX_LAYERS:
            raise EcError(EC_ERR_ARG, f"{what}: {k} layers, not within 1 .. EC_COMPOSITE_MAX_LAYERS ({EC_COMPOSITE_MAX_LAYERS})")
        masks = list(masks) if masks is not None else [None] * k
        if len(masks) != k:
            raise EcError(EC_ERR_ARG, f"{what}: {len(masks)} masks for {k} layers")
        ct, lens = layers[0].ct, layers[0].lens
        for i, b in enumerate(layers):
            if b.ct != ct:
                raise EcError(EC_ERR_ARG, f"{what}: layer {i} is {B.CT_NAMES[b.ct]}, layer 0 {B.CT_NAMES[ct]}: cast the stack to one cell type first")
            if b.lens != lens or (masks[i] is not None and masks[i].lens != lens):
                raise EcError(EC_ERR_ARG, f"{what}: layer {i} or its mask is not sharded like layer 0")
        if isinstance(min_count, bool) or not isinstance(min_count, int) or not 1 <= min_count <= k:
            raise EcError(EC_ERR_ARG, f"{what}: min_count {min_count!r} is not within 1 .. {k}, the number of layers")
        masked = any(m is not None for m in masks)
        out = self.alloc(result_type(ct), lens)
        om = self.alloc(B.UInt8, lens) if masked else None
        ax = self.alloc(B.UInt8, lens) if aux else None
        p = (PVP * k)(*[C.cast(b.ptrs, PVP) for b in layers])
        m = (PVP * k)(*[C.cast(b.ptrs, PVP) if b is not None else PVP() for b in masks]) if masked else None
        check(call(ct, p, m, k, (C.c_size_t * self.n)(*lens), out.ptrs, om.ptrs if masked else None, ax.ptrs if aux else None))
        res = (out, om) if masked else (out,)
        res = res + (ax,) if aux else res
        return res[0] if len(res) == 1 else res

    def composite(self, layers, op="first", min_count: int = 1, aux: bool = False, masks=None):
        """`composite` on every shard, fire-and-forget: `layers` up to 64 identically sharded buffers of one cell type, `masks` (optional)
        one sharded mask or None per layer.  Returns the sharded result, `(result, mask)` when a layer has a mask, and with `aux` the
        sharded UInt8 aux buffer as the last element."""
        o = B._composite_op(op)
        return self._stack_call("composite", layers, masks, min_count, aux, lambda ct: lib().ec_composite_result_type(o, ct),
                                lambda ct, p, m, k, n, dst, dm, ax: lib().ec_sharded_composite(self.handle, o, ct, p, m, k, n, min_count, dst, dm, ax))

    def composite_rank(self, layers, q=(1, 2), method="lower", min_count: int = 1, aux: bool = False, masks=None):
        """`composite_rank` on every shard, fire-and-forget: the per-cell order statistic (q = (num, den); (1, 2) the median) of up to 64
        identically sharded buffers of one cell type, `masks` (optional) one sharded mask or None per layer.  Returns what `composite`
        returns: the sharded result, `(result, mask)` when a layer has a mask, and with `aux` the sharded UInt8 aux buffer last."""
        num, den, mth = B._rank_args(q, method)
        return self._stack_call("composite_rank", layers, masks, min_count, aux, lambda ct: ct,
                                lambda ct, p, m, k, n, dst, dm, ax: lib().ec_sharded_composite_rank(self.handle, ct, p, m, k, n, num, den, mth, min_count,
                                                                                                    dst, dm, ax))

    def program(self, streams, scalars, steps, masks=None):
        """An expression program (`fused.program`: steps `(op, a, b, dst)`) on every shard, fire-and-forget: `streams` up to four
        identically sharded buffers, `masks` (optional) one sharded mask per stream.  Returns the f64 result, or
        `(result, mask)` with `masks`."""
        from ._ffi import EcExprStep, PVP
        lens = streams[0].lens
        assert all(b.lens == lens for b in streams), "operands must be sharded identically"
        k = len(streams)
        dt = (C.c_uint8 * k)(*[b.ct for b in streams])
        p = (PVP * k)(*[C.cast(b.ptrs, PVP) for b in streams])
        m = (PVP * k)(*[C.cast(b.ptrs, PVP) for b in masks]) if masks is not None else None
        sc = (EcValue * max(1, len(scalars)))(*[B.CellValue.new(x).to_ec() for x in scalars])
        st = (EcExprStep * len(steps))(*[EcExprStep(*q) for q in steps])
        out = self.alloc(B.Float64, lens)
        om = self.alloc(B.UInt8, lens) if masks is not None else None
        check(lib().ec_sharded_expr(self.handle, dt, p, m, k, sc, len(scalars), st, len(steps), (C.c_size_t * self.n)(*lens), out.ptrs,
                                    om.ptrs if om is not None else None))
        return out if om is None else (out, om)

    def program_min_max(self, streams, scalars, steps, masks=None):
        """`(min, max)` of a program's result over the whole sharded raster without the raster (`ec_sharded_expr_min_max`)."""
        from ._ffi import EcExprStep, PVP
        lens = streams[0].lens
        assert all(b.lens == lens for b in streams), "operands must be sharded identically"
        k = len(streams)
        dt = (C.c_uint8 * k)(*[b.ct for b in streams])
        p = (PVP * k)(*[C.cast(b.ptrs, PVP) for b in streams])
        m = (PVP * k)(*[C.cast(b.ptrs, PVP) for b in masks]) if masks is not None else None
        sc = (EcValue * max(1, len(scalars)))(*[B.CellValue.new(x).to_ec() for x in scalars])
        st = (EcExprStep * len(steps))(*[EcExprStep(*q) for q in steps])
        mn, mx = EcValue(), EcValue()
        check(lib().ec_sharded_expr_min_max(self.handle, dt, p, m, k, sc, len(scalars), st, len(steps), (C.c_size_t * self.n)(*lens),
                                            C.byref(mn), C.byref(mx)))
        return B.CellValue.from_ec(mn), B.CellValue.from_ec(mx)

    def program_host(self, arrays, scalars, steps, rows: int, cols: int, nodata=None, out_nodata=None, want_mask=False, chunk_cells: int = 0):
        """`fused.program_host` / `program_host_masked` over all the GPUs of the group: the row-blocks of the host arrays
        (rows x cols cells each) stream through their own device's PCIe link side by side (`ec_sharded_host_expr`)."""
        import numpy as np
        from ._ffi import EcExprStep
        arrays = [np.ascontiguousarray(a).reshape(-1) for a in arrays]
        n = rows * cols
        assert all(a.size >= n for a in arrays)
        k = len(arrays)
        cts = [B.cell_type_of(a.dtype) for a in arrays]
        dt = (C.c_uint8 * k)(*cts)
        p = (C.c_void_p * k)(*[a.ctypes.data for a in arrays])
        nd = None
        if nodata is not None:
            nds = [None if v is None else B.CellValue(ct, v).to_ec() for ct, v in zip(cts, nodata)]
            nd = (C.POINTER(EcValue) * k)(*[C.pointer(v) if v is not None else C.POINTER(EcValue)() for v in nds])
        sc = (EcValue * max(1, len(scalars)))(*[B.CellValue.new(x).to_ec() for x in scalars])
        st = (EcExprStep * len(steps))(*[EcExprStep(*q) for q in steps])
        out = np.empty(n, dtype=np.float64)
        mask = np.empty(n, dtype=np.uint8) if want_mask else None
        ond = C.c_double(out_nodata) if out_nodata is not None else None
        check(lib().ec_sharded_host_expr(self.handle, dt, p, nd, k, sc, len(scalars), st, len(steps), rows, cols, out.ctypes.data,
                                         C.byref(ond) if ond is not None else None, mask.ctypes.data if mask is not None else None, chunk_cells))
        return (out, mask.astype(bool)) if want_mask else out

    def min_max(self, sb: ShardedBuffer, mask: ShardedBuffer = None):
        mn, mx = EcValue(), EcValue()
        check(lib().ec_sharded_min_max(self.handle, sb.ct, sb.ptrs, mask.ptrs if mask is not None else None,
                                       (C.c_size_t * self.n)(*sb.lens), C.byref(mn), C.byref(mx)))
        return B.CellValue.from_ec(mn), B.CellValue.from_ec(mx)

    def stats(self, sb: ShardedBuffer, mask: ShardedBuffer = None) -> "B.Stats":
        """`CellBuffer.stats` of the whole sharded raster: one record per shard, folded on the host in shard order (no collective)."""
        out = EcStats()
        check(lib().ec_sharded_stats(self.handle, sb.ct, sb.ptrs, mask.ptrs if mask is not None else None,
                                     (C.c_size_t * self.n)(*sb.lens), C.byref(out)))
        return B.Stats.from_ec(out)

    def _zonal_raw(self, what: str, cap_name: str, fn: str, sb: ShardedBuffer, zones: ShardedBuffer, n_zones, mask: ShardedBuffer):
        """The `n_zones` ec_stats of the whole sharded raster as the library's `fn` (ec_sharded_zonal_stats, ec_sharded_zonal_table)
        leaves them; `cap_name`: the family's cap on n_zones."""
        import numpy as np
        from . import _ffi
        if list(zones.lens) != list(sb.lens) or (mask is not None and list(mask.lens) != list(sb.lens)):
            raise _ffi.EcError(_ffi.EC_ERR_ARG, f"{what}: the zone raster or the mask is not sharded like the values")
        n_zones = B._check_n_zones(what, cap_name, getattr(_ffi, cap_name), n_zones)  # a numpy K (of `regions`) as CellBuffer's forms take it
        raw = np.empty(n_zones, dtype=B._EC_STATS_DTYPE)
        check(getattr(lib(), fn)(self.handle, sb.ct, sb.ptrs, mask.ptrs if mask is not None else None, zones.ct, zones.ptrs,
                                 (C.c_size_t * self.n)(*sb.lens), n_zones, raw.ctypes.data))
        return raw

    def zonal_stats(self, sb: ShardedBuffer, zones: ShardedBuffer, n_zones: int, mask: ShardedBuffer = None) -> list:
        """`CellBuffer.zonal_stats` of the whole sharded raster: every shard's `n_zones` records, zone by zone folded on the host in
        shard order (no collective).  `zones`: the zone raster (UInt8, UInt16 or Int32), sharded like `sb`."""
        return B._stats_list(self._zonal_raw("zonal_stats", "EC_ZONAL_MAX_ZONES", "ec_sharded_zonal_stats", sb, zones, n_zones, mask))

    def zonal_table(self, sb: ShardedBuffer, zones: ShardedBuffer, n_zones: int, mask: ShardedBuffer = None):
        """`CellBuffer.zonal_table` of the whole sharded raster (ec_sharded_zonal_table): up to EC_ZONAL_TABLE_MAX_ZONES zones, every
        shard's records folded zone by zone on the host in shard order; one numpy structured array of `n_zones` rows."""
        return B.stats_table(self._zonal_raw("zonal_table", "EC_ZONAL_TABLE_MAX_ZONES", "ec_sharded_zonal_table", sb, zones, n_zones, mask), sb.ct)

    def counts(self, mask: ShardedBuffer) -> tuple[int, int]:
        t, f = C.c_uint64(), C.c_uint64()
        check(lib().ec_sharded_counts(self.handle, mask.ptrs, (C.c_size_t * self.n)(*mask.lens), C.byref(t), C.byref(f)))
        return t.value, f.value
