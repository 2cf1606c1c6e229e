//! Row-block sharding across the GPUs of one node.
//!
//! Element-wise work is local to a shard; only the two scalar statistics cross GPUs — `min_max` as an
//! all-reduce(MAX) of two order-preserving int64 keys, `counts` as an all-reduce(SUM) of two uint64, both over
//! xGMI through RCCL.  Two shapes:
//!
//! * one process per GPU — [`Communicator`]: rank 0 makes a [`UniqueId`], the host program hands its 128 bytes to
//!   the other ranks, every rank joins; then [`Communicator::min_max`] / [`Communicator::counts`] on its own shard;
//! * one process driving all GPUs — [`ShardGroup`]: per device a launch thread, a stream and a communicator of
//!   the clique, owned by the library; [`ShardGroup::scatter`] cuts a host `Vec` into row-blocks.
//!
//! Neither takes a foreign `ncclComm_t`: the library builds its communicators itself.
use crate::device::stream;
use crate::error::{check, must, Result};
use crate::ffi::*;
use crate::{BufferOps, CastMode, CellBuffer, CellEncoding, CellType, CellValue, Cmp, CompositeOp, RankFraction, RankMethod, Stats};
#[cfg(feature = "masked")]
use crate::Mask;
use std::os::raw::c_void;
use std::ptr;

/// Contiguous cell range `(offset, len)` of shard `shard` of `n_shards` for an `n_rows x n_cols` raster: rows
/// `[g*R/G, (g+1)*R/G)`, the first `R mod G` shards one row longer.
pub fn shard_range(n_rows: u64, n_cols: u64, shard: u32, n_shards: u32) -> (u64, u64) {
    let (mut off, mut len) = (0u64, 0u64);
    must(unsafe { ec_shard_range(n_rows, n_cols, shard, n_shards, &mut off, &mut len) }, "ec_shard_range");
    (off, len)
}

/// The 128 bytes rank 0 hands to the other ranks (a file, a socket, an environment variable ...).
#[derive(Copy, Clone)]
pub struct UniqueId(pub [u8; 128]);

impl UniqueId {
    /// Call on rank 0 only.
    pub fn new() -> Result<Self> {
        let mut uid = ec_comm_uid { bytes: [0; 128] };
        check(unsafe { ec_comm_get_unique_id(&mut uid) })?;
        Ok(UniqueId(uid.bytes.map(|b| b as u8)))
    }
}

/// This rank's end of an RCCL communicator (one process per GPU), with its 32-byte device payload slot.
pub struct Communicator {
    comm: ec_comm,
    payload: *mut c_void,
}

impl Communicator {
    /// Blocks until all `n_ranks` ranks have joined; the calling thread's device ([`crate::init`]) is this rank's GPU.
    pub fn join(uid: &UniqueId, n_ranks: i32, rank: i32) -> Result<Self> {
        let raw = ec_comm_uid { bytes: uid.0.map(|b| b as std::os::raw::c_char) };
        let mut comm: ec_comm = ptr::null_mut();
        check(unsafe { ec_comm_init_rank(&raw, n_ranks, rank, &mut comm) })?;
        let mut payload = ptr::null_mut();
        check(unsafe { ec_alloc(&mut payload, 32) })?;
        Ok(Self { comm, payload })
    }

    /// Global `min_max` of the raster whose local row-block is `local` (collective: every rank calls it).
    #[cfg(feature = "masked")]
    pub fn min_max(&self, local: &CellBuffer, mask: Option<&Mask>) -> (CellValue, CellValue) {
        self.min_max_raw(local, mask.map_or(ptr::null(), |m| m.dev_ptr()))
    }
    #[cfg(not(feature = "masked"))]
    pub fn min_max(&self, local: &CellBuffer) -> (CellValue, CellValue) {
        self.min_max_raw(local, ptr::null())
    }
    fn min_max_raw(&self, local: &CellBuffer, mask: *const u8) -> (CellValue, CellValue) {
        let keys = self.payload as *mut i64;
        must(unsafe { ec_min_max_keys(local.ct as u8, local.dev_ptr(), mask, local.len(), keys, stream()) }, "ec_min_max_keys");
        must(unsafe { ec_allreduce_min_max_keys(self.comm, keys, stream()) }, "ec_allreduce_min_max_keys");
        let mut host = [0i64; 2];
        must(unsafe { ec_download(host.as_mut_ptr() as *mut c_void, keys as *const c_void, 16, stream()) }, "ec_download");
        decode_keys(local.ct, &host)
    }

    /// Global `(data, nodata)` counts of a row-sharded mask (collective).
    #[cfg(feature = "masked")]
    pub fn counts(&self, local: &Mask) -> (u64, u64) {
        let c = self.payload as *mut u64;
        must(unsafe { ec_mask_counts_device(local.dev_ptr(), local.len(), c, stream()) }, "ec_mask_counts_device");
        must(unsafe { ec_allreduce_counts(self.comm, c, stream()) }, "ec_allreduce_counts");
        let mut host = [0u64; 2];
        must(unsafe { ec_download(host.as_mut_ptr() as *mut c_void, c as *const c_void, 16, stream()) }, "ec_download");
        (host[0], host[1])
    }
}

impl Drop for Communicator {
    fn drop(&mut self) {
        unsafe {
            ec_free(self.payload);
            ec_comm_destroy(self.comm);
        }
    }
}

fn decode_keys(ct: CellType, keys: &[i64; 2]) -> (CellValue, CellValue) {
    let (mut mn, mut mx) = (CellValue::UInt8(0).to_ffi(), CellValue::UInt8(0).to_ffi());
    must(unsafe { ec_min_max_decode(ct as u8, keys.as_ptr(), &mut mn, &mut mx) }, "ec_min_max_decode");
    (CellValue::from_ffi(&mn), CellValue::from_ffi(&mx))
}

/// One process driving `n` GPUs: shard `i` of every sharded buffer lives on device `i` of the group.
pub struct ShardGroup {
    g: *mut ec_shard_group,
    n: usize,
}

/// A raster cut into row-blocks, one device block per GPU of a [`ShardGroup`].
pub struct ShardedCellBuffer<'g> {
    group: &'g ShardGroup,
    ct: CellType,
    ptrs: Vec<*mut c_void>,
    lens: Vec<usize>,
}

impl ShardGroup {
    /// `devices` are HIP device indices; RCCL needs them distinct.  Initialises each device.
    pub fn new(devices: &[i32]) -> Result<Self> {
        let mut g = ptr::null_mut();
        check(unsafe { ec_shard_group_create(devices.as_ptr(), devices.len() as i32, EC_GROUP_RCCL, &mut g) })?;
        Ok(Self { g, n: devices.len() })
    }

    pub fn len(&self) -> usize {
        self.n
    }

    pub fn is_empty(&self) -> bool {
        self.n == 0
    }

    /// Cut `data` (row-major, `n_rows x n_cols`) into contiguous row-blocks and upload block `i` to device `i`.
    pub fn scatter<T: CellEncoding>(&self, data: &[T], n_rows: u64, n_cols: u64) -> Result<ShardedCellBuffer<'_>> {
        assert_eq!(data.len() as u64, n_rows * n_cols);
        let sz = std::mem::size_of::<T>();
        let ranges: Vec<(u64, u64)> = (0..self.n).map(|i| shard_range(n_rows, n_cols, i as u32, self.n as u32)).collect();
        let lens: Vec<usize> = ranges.iter().map(|r| r.1 as usize).collect();
        let bytes: Vec<usize> = lens.iter().map(|l| l * sz).collect();
        let offs: Vec<usize> = ranges.iter().map(|r| r.0 as usize * sz).collect();
        let mut ptrs: Vec<*mut c_void> = vec![ptr::null_mut(); self.n];
        check(unsafe { ec_sharded_alloc(self.g, bytes.as_ptr(), ptrs.as_mut_ptr()) })?;
        check(unsafe { ec_sharded_upload(self.g, ptrs.as_ptr(), data.as_ptr() as *const c_void, offs.as_ptr(), bytes.as_ptr()) })?;
        Ok(ShardedCellBuffer { group: self, ct: T::cell_type(), ptrs, lens })
    }

    /// Wait until everything queued so far has been issued and every shard's stream has drained.  The element-wise
    /// sharded calls are fire-and-forget: a failure inside one of them (a launch error) is reported here, once.
    pub fn sync(&self) -> Result<()> {
        check(unsafe { ec_shard_group_sync(self.g) })
    }
}

impl Drop for ShardGroup {
    fn drop(&mut self) {
        unsafe { ec_shard_group_destroy(self.g) };
    }
}

impl ShardedCellBuffer<'_> {
    pub fn cell_type(&self) -> CellType {
        self.ct
    }

    pub fn len(&self) -> usize {
        self.lens.iter().sum()
    }

    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }

    fn const_ptrs(&self) -> Vec<*const c_void> {
        self.ptrs.iter().map(|p| *p as *const c_void).collect()
    }

    fn alloc_like(&self, ct: CellType) -> Result<Self> {
        let bytes: Vec<usize> = self.lens.iter().map(|l| l * ct.size_of()).collect();
        let mut ptrs: Vec<*mut c_void> = vec![ptr::null_mut(); self.lens.len()];
        check(unsafe { ec_sharded_alloc(self.group.g, bytes.as_ptr(), ptrs.as_mut_ptr()) })?;
        Ok(Self { group: self.group, ct, ptrs, lens: self.lens.clone() })
    }

    /// `self op rhs` on every shard (no communication); both rasters must be cut the same way.
    pub fn binop(&self, op: ec_op, rhs: &Self) -> Result<Self> {
        assert_eq!(self.lens, rhs.lens, "operands must be sharded identically");
        let out = self.alloc_like(CellType::Float64)?;
        let outs: Vec<*mut f64> = out.ptrs.iter().map(|p| *p as *mut f64).collect();
        check(unsafe {
            ec_sharded_binop(self.group.g, op, self.ct as u8, self.const_ptrs().as_ptr(), rhs.ct as u8, rhs.const_ptrs().as_ptr(),
                             self.lens.as_ptr(), outs.as_ptr())
        })?;
        Ok(out)
    }

    /// [`CellBuffer::compare`] on every shard (no communication): a `UInt8` raster of 0 / 1 bytes cut the same way.
    pub fn compare(&self, rel: Cmp, rhs: &Self) -> Result<Self> {
        assert_eq!(self.lens, rhs.lens, "operands must be sharded identically");
        let out = self.alloc_like(CellType::UInt8)?;
        let outs: Vec<*mut u8> = out.ptrs.iter().map(|p| *p as *mut u8).collect();
        check(unsafe {
            ec_sharded_compare(self.group.g, rel as i32, self.ct as u8, self.const_ptrs().as_ptr(), ptr::null(), rhs.ct as u8,
                               rhs.const_ptrs().as_ptr(), ptr::null(), self.lens.as_ptr(), outs.as_ptr())
        })?;
        Ok(out)
    }

    /// [`CellBuffer::compare_scalar`] on every shard.
    pub fn compare_scalar<R: Into<CellValue>>(&self, rel: Cmp, rhs: R) -> Result<Self> {
        let out = self.alloc_like(CellType::UInt8)?;
        let outs: Vec<*mut u8> = out.ptrs.iter().map(|p| *p as *mut u8).collect();
        let v = rhs.into().to_ffi();
        check(unsafe {
            ec_sharded_compare_scalar(self.group.g, rel as i32, self.ct as u8, self.const_ptrs().as_ptr(), ptr::null(), self.lens.as_ptr(), &v,
                                      outs.as_ptr())
        })?;
        Ok(out)
    }

    /// [`CellBuffer::cast`] on every shard (no communication).
    pub fn cast(&self, cell_type: CellType, mode: CastMode) -> Result<Self> {
        let out = self.alloc_like(cell_type)?;
        check(unsafe {
            ec_sharded_cast(self.group.g, mode as i32, self.ct as u8, self.const_ptrs().as_ptr(), cell_type as u8, out.ptrs.as_ptr(), self.lens.as_ptr())
        })?;
        Ok(out)
    }

    /// [`CellBuffer::to_scaled`] on every shard.
    pub fn to_scaled(&self, cell_type: CellType, scale: f64, offset: f64) -> Result<Self> {
        let out = self.alloc_like(cell_type)?;
        check(unsafe {
            ec_sharded_cast_scaled(self.group.g, self.ct as u8, self.const_ptrs().as_ptr(), ptr::null(), self.lens.as_ptr(), scale, offset,
                                   cell_type as u8, ptr::null(), out.ptrs.as_ptr())
        })?;
        Ok(out)
    }

    /// [`MaskedCellBuffer::to_scaled`] on every shard: `mask` is a `UInt8` raster of 0 / 1 bytes cut the same way, and a cell whose
    /// mask byte is 0 receives `nodata` (a value of type `cell_type`).
    pub fn to_scaled_masked(&self, cell_type: CellType, scale: f64, offset: f64, mask: &Self, nodata: CellValue) -> Result<Self> {
        assert_eq!(self.lens, mask.lens, "the mask must be sharded like its operand");
        let out = self.alloc_like(cell_type)?;
        let masks: Vec<*const u8> = mask.ptrs.iter().map(|p| *p as *const u8).collect();
        let marker = nodata.to_ffi();
        check(unsafe {
            ec_sharded_cast_scaled(self.group.g, self.ct as u8, self.const_ptrs().as_ptr(), masks.as_ptr(), self.lens.as_ptr(), scale, offset,
                                   cell_type as u8, &marker, out.ptrs.as_ptr())
        })?;
        Ok(out)
    }

    /// [`CellBuffer::composite`] of identically sharded layers on every shard (no communication).  `masks`: empty, or one entry per
    /// layer — a `UInt8` raster of 0 / 1 bytes cut the same way, or `None` for a layer without a mask.  Returns the result, its mask
    /// when a layer has one, and the `UInt8` raster of where each cell came from.
    pub fn composite(layers: &[&Self], masks: &[Option<&Self>], op: CompositeOp, min_count: u32) -> Result<(Self, Option<Self>, Self)> {
        assert!(!layers.is_empty() && layers.len() <= EC_COMPOSITE_MAX_LAYERS, "a stack holds 1 .. {EC_COMPOSITE_MAX_LAYERS} layers, not {}", layers.len());
        assert!(masks.is_empty() || masks.len() == layers.len(), "one mask entry per layer");
        let first = layers[0];
        for l in layers {
            assert!(l.ct == first.ct && l.lens == first.lens, "the layers of a stack share a cell type and a sharding");
        }
        let cell_cols: Vec<Vec<*const c_void>> = layers.iter().map(|l| l.const_ptrs()).collect();
        let cells: Vec<*const *const c_void> = cell_cols.iter().map(|c| c.as_ptr()).collect();
        let mask_cols: Vec<Option<Vec<*const u8>>> = masks.iter().map(|m| m.map(|b| b.ptrs.iter().map(|p| *p as *const u8).collect())).collect();
        let mask_ptrs: Vec<*const *const u8> = mask_cols.iter().map(|c| c.as_ref().map_or(ptr::null(), |v| v.as_ptr())).collect();
        let masked = masks.iter().any(|m| m.is_some());
        let out = first.alloc_like(op.result_type(first.ct))?;
        let out_mask = if masked { Some(first.alloc_like(CellType::UInt8)?) } else { None };
        let source = first.alloc_like(CellType::UInt8)?;
        let bytes = |b: &Self| -> Vec<*mut u8> { b.ptrs.iter().map(|p| *p as *mut u8).collect() };
        let (mask_out, source_out) = (out_mask.as_ref().map(bytes), bytes(&source));
        check(unsafe {
            ec_sharded_composite(first.group.g, op as i32, first.ct as u8, cells.as_ptr(), if masked { mask_ptrs.as_ptr() } else { ptr::null() },
                                 layers.len() as i32, first.lens.as_ptr(), min_count, out.ptrs.as_ptr(),
                                 mask_out.as_ref().map_or(ptr::null(), |v| v.as_ptr()), source_out.as_ptr())
        })?;
        Ok((out, out_mask, source))
    }

    /// [`CellBuffer::composite_rank`] of identically sharded layers on every shard (no communication); `masks` and the three results as
    /// for [`ShardedCellBuffer::composite`].
    pub fn composite_rank(layers: &[&Self], masks: &[Option<&Self>], q: RankFraction, method: RankMethod, min_count: u32) -> Result<(Self, Option<Self>, Self)> {
        assert!(!layers.is_empty() && layers.len() <= EC_COMPOSITE_MAX_LAYERS, "a stack holds 1 .. {EC_COMPOSITE_MAX_LAYERS} layers, not {}", layers.len());
        assert!(masks.is_empty() || masks.len() == layers.len(), "one mask entry per layer");
        let first = layers[0];
        for l in layers {
            assert!(l.ct == first.ct && l.lens == first.lens, "the layers of a stack share a cell type and a sharding");
        }
        let cell_cols: Vec<Vec<*const c_void>> = layers.iter().map(|l| l.const_ptrs()).collect();
        let cells: Vec<*const *const c_void> = cell_cols.iter().map(|c| c.as_ptr()).collect();
        let mask_cols: Vec<Option<Vec<*const u8>>> = masks.iter().map(|m| m.map(|b| b.ptrs.iter().map(|p| *p as *const u8).collect())).collect();
        let mask_ptrs: Vec<*const *const u8> = mask_cols.iter().map(|c| c.as_ref().map_or(ptr::null(), |v| v.as_ptr())).collect();
        let masked = masks.iter().any(|m| m.is_some());
        let out = first.alloc_like(first.ct)?;
        let out_mask = if masked { Some(first.alloc_like(CellType::UInt8)?) } else { None };
        let source = first.alloc_like(CellType::UInt8)?;
        let bytes = |b: &Self| -> Vec<*mut u8> { b.ptrs.iter().map(|p| *p as *mut u8).collect() };
        let (mask_out, source_out) = (out_mask.as_ref().map(bytes), bytes(&source));
        check(unsafe {
            ec_sharded_composite_rank(first.group.g, first.ct as u8, cells.as_ptr(), if masked { mask_ptrs.as_ptr() } else { ptr::null() },
                                      layers.len() as i32, first.lens.as_ptr(), q.num, q.den, method as i32, min_count, out.ptrs.as_ptr(),
                                      mask_out.as_ref().map_or(ptr::null(), |v| v.as_ptr()), source_out.as_ptr())
        })?;
        Ok((out, out_mask, source))
    }

    /// `BufferOps::min_max` of the whole raster: per-shard keys, one all-reduce over xGMI, decode.
    pub fn min_max(&self) -> Result<(CellValue, CellValue)> {
        let (mut mn, mut mx) = (CellValue::UInt8(0).to_ffi(), CellValue::UInt8(0).to_ffi());
        check(unsafe {
            ec_sharded_min_max(self.group.g, self.ct as u8, self.const_ptrs().as_ptr(), ptr::null(), self.lens.as_ptr(), &mut mn, &mut mx)
        })?;
        Ok((CellValue::from_ffi(&mn), CellValue::from_ffi(&mx)))
    }

    /// [`CellBuffer::stats`] of the whole raster: one record per shard, folded on the host in shard order (no collective).
    /// `mask`: a `UInt8` raster of 0 / 1 bytes cut the same way; a cell counts iff its byte is non-zero.
    pub fn stats(&self, mask: Option<&Self>) -> Result<Stats> {
        if let Some(m) = mask {
            assert_eq!(m.ct, CellType::UInt8, "a mask is UInt8 bytes");
            assert_eq!(m.lens, self.lens, "the mask must be sharded identically");
        }
        let masks: Vec<*const u8> = mask.map_or(Vec::new(), |m| m.ptrs.iter().map(|p| *p as *const u8).collect());
        let mut out = Stats::blank();
        check(unsafe {
            ec_sharded_stats(self.group.g, self.ct as u8, self.const_ptrs().as_ptr(), if mask.is_some() { masks.as_ptr() } else { ptr::null() },
                             self.lens.as_ptr(), &mut out as *mut ec_stats as *mut c_void)
        })?;
        Ok(Stats::from_ffi(&out))
    }

    /// [`CellBuffer::zonal_stats`] of the whole raster: every shard's `n_zones` records, zone by zone folded on the host in shard order
    /// (no collective).  `zones`: the zone raster cut the same way; `mask` as for [`Self::stats`].
    pub fn zonal_stats(&self, zones: &Self, n_zones: usize, mask: Option<&Self>) -> Result<Vec<Stats>> {
        assert_eq!(zones.lens, self.lens, "the zone raster must be sharded identically");
        assert!((1..=EC_ZONAL_MAX_ZONES).contains(&n_zones), "1 .. {EC_ZONAL_MAX_ZONES} zones, not {n_zones}");
        if let Some(m) = mask {
            assert_eq!(m.ct, CellType::UInt8, "a mask is UInt8 bytes");
            assert_eq!(m.lens, self.lens, "the mask must be sharded identically");
        }
        let masks: Vec<*const u8> = mask.map_or(Vec::new(), |m| m.ptrs.iter().map(|p| *p as *const u8).collect());
        let mut out = vec![Stats::blank(); n_zones];
        check(unsafe {
            ec_sharded_zonal_stats(self.group.g, self.ct as u8, self.const_ptrs().as_ptr(), if mask.is_some() { masks.as_ptr() } else { ptr::null() },
                                   zones.ct as u8, zones.const_ptrs().as_ptr(), self.lens.as_ptr(), n_zones as i32, out.as_mut_ptr() as *mut c_void)
        })?;
        Ok(out.iter().map(Stats::from_ffi).collect())
    }

    /// [`CellBuffer::zonal_table`] of the whole raster (`ec_sharded_zonal_table`): up to `EC_ZONAL_TABLE_MAX_ZONES` zones, the fold
    /// of [`Self::zonal_stats`] unchanged.
    pub fn zonal_table(&self, zones: &Self, n_zones: usize, mask: Option<&Self>) -> Result<Vec<Stats>> {
        assert_eq!(zones.lens, self.lens, "the zone raster must be sharded identically");
        assert!((1..=EC_ZONAL_TABLE_MAX_ZONES).contains(&n_zones), "1 .. {EC_ZONAL_TABLE_MAX_ZONES} zones, not {n_zones}");
        if let Some(m) = mask {
            assert_eq!(m.ct, CellType::UInt8, "a mask is UInt8 bytes");
            assert_eq!(m.lens, self.lens, "the mask must be sharded identically");
        }
        let masks: Vec<*const u8> = mask.map_or(Vec::new(), |m| m.ptrs.iter().map(|p| *p as *const u8).collect());
        let mut out = vec![Stats::blank(); n_zones];
        check(unsafe {
            ec_sharded_zonal_table(self.group.g, self.ct as u8, self.const_ptrs().as_ptr(), if mask.is_some() { masks.as_ptr() } else { ptr::null() },
                                   zones.ct as u8, zones.const_ptrs().as_ptr(), self.lens.as_ptr(), n_zones as i32, out.as_mut_ptr() as *mut c_void)
        })?;
        Ok(out.iter().map(Stats::from_ffi).collect())
    }

    /// [`CellBuffer::reclassify`] on every shard (no communication, fire-and-forget).  `tables`: the table's record on every
    /// shard's device — a `UInt8` buffer of `EC_RECLASS_TABLE_BYTES` per shard, uploaded by the caller ([`ShardGroup::scatter`] of the
    /// record's bytes repeated, one row of `EC_RECLASS_TABLE_BYTES` cells per shard) — for rasters of this cell type, results of `result_type`; `mask`: a `UInt8` raster of 0 / 1 bytes cut the
    /// same way, given iff the table was built with a nodata value.  Returns the result and, when asked for, its mask.
    pub fn reclassify(&self, tables: &Self, result_type: CellType, mask: Option<&Self>, want_mask: bool) -> Result<(Self, Option<Self>)> {
        assert!(tables.ct == CellType::UInt8 && tables.lens.iter().all(|l| *l == EC_RECLASS_TABLE_BYTES), "one record per shard");
        if let Some(m) = mask {
            assert_eq!(m.ct, CellType::UInt8, "a mask is UInt8 bytes");
            assert_eq!(m.lens, self.lens, "the mask must be sharded identically");
        }
        let out = self.alloc_like(result_type)?;
        let om = if want_mask { Some(self.alloc_like(CellType::UInt8)?) } else { None };
        let masks: Vec<*const u8> = mask.map_or(Vec::new(), |m| m.ptrs.iter().map(|p| *p as *const u8).collect());
        let out_masks: Vec<*mut u8> = om.as_ref().map_or(Vec::new(), |m| m.ptrs.iter().map(|p| *p as *mut u8).collect());
        check(unsafe {
            ec_sharded_reclass(self.group.g, self.ct as u8, self.const_ptrs().as_ptr(), if mask.is_some() { masks.as_ptr() } else { ptr::null() },
                               self.lens.as_ptr(), result_type as u8, tables.const_ptrs().as_ptr(), out.ptrs.as_ptr(),
                               if want_mask { out_masks.as_ptr() } else { ptr::null() })
        })?;
        Ok((out, om))
    }

    /// Gather the shards back into one host `Vec` (the type must be the buffer's own cell type).
    pub fn to_vec<T: CellEncoding + Default>(&self) -> Result<Vec<T>> {
        assert_eq!(self.ct, T::cell_type());
        let sz = std::mem::size_of::<T>();
        let mut out = vec![T::default(); self.len()];
        let bytes: Vec<usize> = self.lens.iter().map(|l| l * sz).collect();
        let mut offs = Vec::with_capacity(self.lens.len());
        let mut acc = 0usize;
        for l in &self.lens {
            offs.push(acc * sz);
            acc += l;
        }
        check(unsafe {
            ec_sharded_download(self.group.g, out.as_mut_ptr() as *mut c_void, self.const_ptrs().as_ptr(), offs.as_ptr(), bytes.as_ptr())
        })?;
        Ok(out)
    }
}

impl Drop for ShardedCellBuffer<'_> {
    fn drop(&mut self) {
        unsafe {
            ec_shard_group_sync(self.group.g);
            ec_sharded_free(self.group.g, self.ptrs.as_ptr());
        }
    }
}

/// A single-device view, for code that mixes the two shapes: shard `i` of a sharded buffer as a borrowed
/// `(device pointer, len)` pair on device `i`'s stream.
pub fn shard_of<'a>(b: &'a ShardedCellBuffer<'_>, i: usize) -> (*const c_void, usize) {
    (b.ptrs[i] as *const c_void, b.lens[i])
}
