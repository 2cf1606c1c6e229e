//! Raw `extern "C"` declarations of include/erased_cells.h (ABI version 1).
//! Every data pointer is a DEVICE pointer unless the name says `host`.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_void};

pub type ec_status = i32;
pub type ec_dtype = u8; // `CellType as u8` (src/ctype.rs:16)
pub type ec_op = i32;
pub type ec_stream = *mut c_void; // hipStream_t
pub type ec_comm = *mut c_void; // ncclComm_t

/// Mirrors `ec_comm_uid` (ncclUniqueId): 128 opaque bytes rank 0 hands to the other ranks.
#[repr(C)]
#[derive(Copy, Clone)]
pub struct ec_comm_uid {
    pub bytes: [c_char; 128],
}

/// Opaque `ec_shard_group`: one process driving n GPUs.
#[repr(C)]
pub struct ec_shard_group {
    _private: [u8; 0],
}
pub const EC_GROUP_RCCL: u32 = 0;
pub const EC_GROUP_HOST_COMBINE: u32 = 1;
/// Every sharded call waits until all launch threads have issued (the form of rounds 1-2; default: fire-and-forget).
pub const EC_GROUP_BLOCKING_ISSUE: u32 = 2;
/// `ec_shard_fn`: called once per shard on that shard's launch thread.
pub type ec_shard_fn = extern "C" fn(shard: i32, device: i32, stream: ec_stream, user: *mut c_void) -> ec_status;

pub const EC_OK: ec_status = 0;
pub const EC_ERR_NARROWING: ec_status = 1;
pub const EC_ADD: ec_op = 0;
pub const EC_SUB: ec_op = 1;
pub const EC_MUL: ec_op = 2;
pub const EC_DIV: ec_op = 3;
/// `ec_resample`: GDAL's `GRIORA_*` numbers of the algorithms `ec_window_resample` has (it takes them as an `i32`).
pub const EC_RESAMPLE_NEAREST: i32 = 0;
pub const EC_RESAMPLE_BILINEAR: i32 = 1;
pub const EC_RESAMPLE_AVERAGE: i32 = 5;
/// An average reduces an axis by at most this factor per call; chain calls for more.
pub const EC_WINDOW_MAX_REDUCTION: u64 = 64;
/// `ec_cmp`: a relation is the truth table over `Ordering` — bit 0 `Less`, bit 1 `Equal`, bit 2 `Greater` (`ec_compare` takes it as an `i32`).
pub const EC_CMP_LT: i32 = 1;
pub const EC_CMP_EQ: i32 = 2;
pub const EC_CMP_LE: i32 = 3;
pub const EC_CMP_GT: i32 = 4;
pub const EC_CMP_NE: i32 = 5;
pub const EC_CMP_GE: i32 = 6;
/// `ec_cast_mode`: Rust's `as`, or the storing rule — clamp, round half away from zero, saturate (`ec_cast` takes it as an `i32`).
pub const EC_CAST_AS: i32 = 0;
pub const EC_CAST_ROUND: i32 = 1;
/// `ec_focal_op`: what `ec_focal` computes over a footprint (it takes it as an `i32`).
pub const EC_FOCAL_SUM: i32 = 0;
pub const EC_FOCAL_MEAN: i32 = 1;
pub const EC_FOCAL_MIN: i32 = 2;
pub const EC_FOCAL_MAX: i32 = 3;
/// The largest radius of a footprint on either axis: footprints up to 15 x 15.
pub const EC_FOCAL_RADIUS_CAP: u32 = 7;
/// Flags of `ec_focal` / `ec_focal_convolve`: only whole footprints are valid; divide by the weights counted (convolve only).
pub const EC_FOCAL_WHOLE: u32 = 1;
pub const EC_FOCAL_NORMALIZE: u32 = 2;
/// The most cells the footprint of `ec_focal_rank` / `ec_focal_majority` holds: one sorting network (`EC_FOCAL_RANK_MAX_TAPS`).
pub const EC_FOCAL_RANK_MAX_TAPS: u32 = 64;
/// The longest side of a raster `ec_distance` takes (`EC_DISTANCE_MAX_SIDE`) and its `max_sq` of "no limit" (`EC_DISTANCE_UNLIMITED`).
pub const EC_DISTANCE_MAX_SIDE: u64 = 32768;
pub const EC_DISTANCE_UNLIMITED: u32 = 0xFFFF_FFFF;
/// The longest side of a raster `ec_regions` takes (`EC_REGIONS_MAX_SIDE`) and its two numberings (`ec_regions_numbering`, taken as an `i32`).
pub const EC_REGIONS_MAX_SIDE: u64 = 32768;
pub const EC_REGIONS_ROOT: i32 = 0;
pub const EC_REGIONS_DENSE: i32 = 1;
/// The most zones one `ec_zonal_stats_*` call serves (`EC_ZONAL_MAX_ZONES`).
pub const EC_ZONAL_MAX_ZONES: usize = 256;
/// The most zones one `ec_zonal_table_*` / `ec_zonal_lookup` call serves (`EC_ZONAL_TABLE_MAX_ZONES`).
pub const EC_ZONAL_TABLE_MAX_ZONES: usize = 1 << 24;
/// The most breaks one reclass table holds (`EC_RECLASS_MAX_BREAKS`), the size of its record and the flags of the record.
pub const EC_RECLASS_MAX_BREAKS: usize = 255;
pub const EC_RECLASS_TABLE_BYTES: usize = 4384;
pub const EC_RECLASS_HAS_NODATA: u32 = 1;
pub const EC_RECLASS_DROPS: u32 = 2;
/// `ec_composite_op`: what `ec_composite` keeps of a cell's stack of layers (it takes it as an `i32`).
pub const EC_COMPOSITE_FIRST: i32 = 0;
pub const EC_COMPOSITE_LAST: i32 = 1;
pub const EC_COMPOSITE_MIN: i32 = 2;
pub const EC_COMPOSITE_MAX: i32 = 3;
pub const EC_COMPOSITE_SUM: i32 = 4;
pub const EC_COMPOSITE_MEAN: i32 = 5;
/// The tallest stack of one call, and the aux byte of a cell that no layer gave.
pub const EC_COMPOSITE_MAX_LAYERS: usize = 64;
pub const EC_COMPOSITE_NONE: u8 = 255;
/// `ec_rank_method`: which neighbour `ec_composite_rank` keeps (it takes it as an `i32`).
pub const EC_RANK_LOWER: i32 = 0;
pub const EC_RANK_UPPER: i32 = 1;
pub const EC_RANK_MAX_DEN: u32 = 65535;

/// Mirrors `ec_value`: tag + 8-byte payload, 16 bytes.
#[repr(C)]
#[derive(Copy, Clone)]
pub struct ec_value {
    pub dtype: u8,
    pub pad_: [u8; 7],
    pub bits: u64, // the C union; read/written through to_bits()/from_bits() of the primitive
}

/// Mirrors `ec_moments`: the 64-byte record one `ec_stats_device` launch leaves on the device.  `moments` is the C union:
/// kind 0 holds `{sum: i64, sq_lo: u64, sq_hi: u64}`, kind 1 the bits of `{pivot, s1, s2}: f64`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ec_moments {
    pub count: u64,
    pub keys2: [i64; 2],
    pub kind: i32,
    pub dtype: i32,
    pub moments: [u64; 3],
    pub reserved: u64,
}

/// Mirrors `ec_reclass_table`: what `ec_reclass_table_build` writes and `ec_reclass` reads on the device, every byte defined.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ec_reclass_table {
    pub t: i32,
    pub dt: i32,
    pub n_breaks: i32,
    pub n_reached: i32,
    pub flags: u32,
    pub reserved0: u32,
    pub nodata_bits: u64,
    pub reserved1: u64,
    pub thr: [i64; 255],
    pub value_bits: [u64; 256],
    pub valid: [u8; 256],
}

/// Mirrors `ec_stats`: what `ec_stats_fold` makes of one or several records.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ec_stats {
    pub count: u64,
    pub min: ec_value,
    pub max: ec_value,
    pub sum: f64,
    pub mean: f64,
    pub stddev: f64,
}

/// One step of an expression program (`ec_expr`): `reg[dst] = a op b`; `a`, `b` are operand references
/// (`ec_expr_stream(k)`, `ec_expr_reg(k)`, `ec_expr_scalar(k)`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ec_expr_step {
    pub op: i8,
    pub a: i8,
    pub b: i8,
    pub dst: i8,
}
pub const fn ec_expr_stream(k: i8) -> i8 {
    k
}
pub const fn ec_expr_reg(k: i8) -> i8 {
    4 + k
}
pub const fn ec_expr_scalar(k: i8) -> i8 {
    8 + k
}
pub const EC_EXPR_MAX_STREAMS: usize = 4;
pub const EC_EXPR_REGS: usize = 4;
pub const EC_EXPR_MAX_SCALARS: usize = 8;
pub const EC_EXPR_MAX_STEPS: usize = 16;

extern "C" {
    pub fn ec_abi_version() -> i32;
    pub fn ec_init(device: i32) -> ec_status;
    pub fn ec_set_device(device: i32) -> ec_status;
    pub fn ec_get_device(device: *mut i32) -> ec_status;
    pub fn ec_shutdown() -> ec_status;
    pub fn ec_last_error_string() -> *const c_char;
    pub fn ec_last_narrowing(src: *mut ec_dtype, dst: *mut ec_dtype) -> ec_status;
    pub fn ec_device_info(n_cu: *mut i32, hbm_bytes: *mut u64, name: *mut c_char, name_cap: usize) -> ec_status;

    pub fn ec_alloc(dptr: *mut *mut c_void, bytes: usize) -> ec_status;
    pub fn ec_free(dptr: *mut c_void) -> ec_status;
    pub fn ec_alloc_async(dptr: *mut *mut c_void, bytes: usize, s: ec_stream) -> ec_status;
    pub fn ec_free_async(dptr: *mut c_void, s: ec_stream) -> ec_status;
    pub fn ec_free_ordered(dptr: *mut c_void, alloc_stream: ec_stream, last_use_stream: ec_stream) -> ec_status;
    pub fn ec_pool_trim(keep_bytes: usize) -> ec_status;
    pub fn ec_stream_create(out: *mut ec_stream) -> ec_status;
    pub fn ec_prepare_stream(s: ec_stream) -> ec_status;
    pub fn ec_release_stream(s: ec_stream) -> ec_status;
    pub fn ec_stream_destroy(s: ec_stream) -> ec_status;
    pub fn ec_stream_sync(s: ec_stream) -> ec_status;
    pub fn ec_upload(dst_dev: *mut c_void, src_host: *const c_void, bytes: usize, s: ec_stream) -> ec_status;
    pub fn ec_download(dst_host: *mut c_void, src_dev: *const c_void, bytes: usize, s: ec_stream) -> ec_status;
    pub fn ec_copy(dst_dev: *mut c_void, src_dev: *const c_void, bytes: usize, s: ec_stream) -> ec_status;

    pub fn ec_union(a: ec_dtype, b: ec_dtype) -> ec_dtype;
    pub fn ec_can_fit_into(src: ec_dtype, dst: ec_dtype) -> i32;
    pub fn ec_size_of(t: ec_dtype) -> usize;
    pub fn ec_neg_result_type(t: ec_dtype) -> ec_dtype;
    pub fn ec_min_value(t: ec_dtype, out: *mut ec_value) -> ec_status;
    pub fn ec_max_value(t: ec_dtype, out: *mut ec_value) -> ec_status;
    pub fn ec_nodata_default(t: ec_dtype, out: *mut ec_value) -> ec_status;
    pub fn ec_value_convert(v: *const ec_value, dst: ec_dtype, out: *mut ec_value) -> ec_status;
    pub fn ec_value_to_f64(v: *const ec_value) -> f64;

    pub fn ec_binop(op: ec_op, lt: ec_dtype, l: *const c_void, rt: ec_dtype, r: *const c_void, n: usize,
                    out: *mut f64, s: ec_stream) -> ec_status;
    pub fn ec_binop_scalar(op: ec_op, lt: ec_dtype, l: *const c_void, n: usize, rhs: *const ec_value,
                           out: *mut f64, s: ec_stream) -> ec_status;
    pub fn ec_masked_binop(op: ec_op, lt: ec_dtype, l: *const c_void, lmask: *const u8, rt: ec_dtype,
                           r: *const c_void, rmask: *const u8, n: usize, out: *mut f64, out_mask: *mut u8,
                           s: ec_stream) -> ec_status;
    pub fn ec_neg(t: ec_dtype, input: *const c_void, n: usize, out: *mut c_void, s: ec_stream) -> ec_status;
    pub fn ec_convert(st: ec_dtype, src: *const c_void, dt: ec_dtype, dst: *mut c_void, n: usize, s: ec_stream) -> ec_status;
    pub fn ec_fill(t: ec_dtype, dst: *mut c_void, n: usize, value: *const ec_value, s: ec_stream) -> ec_status;

    pub fn ec_min_max(t: ec_dtype, p: *const c_void, mask_or_null: *const u8, n: usize, mn: *mut ec_value,
                      mx: *mut ec_value, s: ec_stream) -> ec_status;
    pub fn ec_min_max_keys(t: ec_dtype, p: *const c_void, mask_or_null: *const u8, n: usize, keys2_dev: *mut i64,
                           s: ec_stream) -> ec_status;
    pub fn ec_min_max_decode(t: ec_dtype, keys2_host: *const i64, mn: *mut ec_value, mx: *mut ec_value) -> ec_status;

    pub fn ec_mask_from_nodata(t: ec_dtype, p: *const c_void, n: usize, nd_or_null: *const ec_value, mask: *mut u8,
                               s: ec_stream) -> ec_status;
    pub fn ec_mask_select(t: ec_dtype, p: *const c_void, mask: *const u8, n: usize, nd_or_null: *const ec_value,
                          out: *mut c_void, s: ec_stream) -> ec_status;
    // per-cell order predicates as masks (impl Ord for CellValue, src/value.rs:248-271) and the pick of cells by a mask
    pub fn ec_compare(rel: i32, lt: ec_dtype, l: *const c_void, lmask_or_null: *const u8, rt: ec_dtype, r: *const c_void,
                      rmask_or_null: *const u8, n: usize, out_mask: *mut u8, s: ec_stream) -> ec_status;
    pub fn ec_compare_scalar(rel: i32, lt: ec_dtype, l: *const c_void, lmask_or_null: *const u8, n: usize,
                             rhs: *const ec_value, out_mask: *mut u8, s: ec_stream) -> ec_status;
    pub fn ec_select(t: ec_dtype, a: *const c_void, b: *const c_void, sel: *const u8, n: usize, out: *mut c_void,
                     s: ec_stream) -> ec_status;
    pub fn ec_masked_select(t: ec_dtype, a: *const c_void, amask: *const u8, b: *const c_void, bmask: *const u8,
                            sel: *const u8, n: usize, out: *mut c_void, out_mask: *mut u8, s: ec_stream) -> ec_status;
    // the cells in a storage cell type, for all 100 type pairs (never EC_ERR_NARROWING), and the storing direction of a scale and offset
    pub fn ec_cast(mode: i32, st: ec_dtype, src: *const c_void, dt: ec_dtype, dst: *mut c_void, n: usize, s: ec_stream) -> ec_status;
    pub fn ec_cast_scaled(st: ec_dtype, src: *const c_void, mask_or_null: *const u8, n: usize, scale: f64, offset: f64,
                          dt: ec_dtype, nodata_or_null: *const ec_value, dst: *mut c_void, s: ec_stream) -> ec_status;
    pub fn ec_mask_and(l: *const u8, r: *const u8, n: usize, out: *mut u8, s: ec_stream) -> ec_status;
    pub fn ec_mask_or(l: *const u8, r: *const u8, n: usize, out: *mut u8, s: ec_stream) -> ec_status;
    pub fn ec_mask_not(m: *const u8, n: usize, out: *mut u8, s: ec_stream) -> ec_status;
    pub fn ec_mask_counts(m: *const u8, n: usize, n_true: *mut u64, n_false: *mut u64, s: ec_stream) -> ec_status;
    pub fn ec_mask_counts_device(m: *const u8, n: usize, counts2_dev: *mut u64, s: ec_stream) -> ec_status;
    pub fn ec_first_difference(t: ec_dtype, l: *const c_void, r: *const c_void, n: usize, index: *mut u64,
                               s: ec_stream) -> ec_status;
    pub fn ec_buffer_cmp(lt: ec_dtype, l: *const c_void, nl: usize, rt: ec_dtype, r: *const c_void, nr: usize,
                         ordering: *mut i32, s: ec_stream) -> ec_status;
    pub fn ec_fused(o1: ec_op, o2: ec_op, o3: ec_op, dt: *const ec_dtype, p: *const *const c_void,
                    scalars_or_null: *const ec_value, n: usize, out: *mut f64, s: ec_stream) -> ec_status;
    pub fn ec_masked_fused(o1: ec_op, o2: ec_op, o3: ec_op, dt: *const ec_dtype, p: *const *const c_void,
                           masks: *const *const u8, scalars_or_null: *const ec_value, n: usize, out: *mut f64,
                           out_mask: *mut u8, s: ec_stream) -> ec_status;
    pub fn ec_expr(dt: *const ec_dtype, p: *const *const c_void, n_streams: i32, scalars: *const ec_value, n_scalars: i32,
                   steps: *const ec_expr_step, n_steps: i32, n: usize, out: *mut f64, s: ec_stream) -> ec_status;
    pub fn ec_masked_expr(dt: *const ec_dtype, p: *const *const c_void, masks: *const *const u8, n_streams: i32,
                          scalars: *const ec_value, n_scalars: i32, steps: *const ec_expr_step, n_steps: i32, n: usize,
                          out: *mut f64, out_mask: *mut u8, s: ec_stream) -> ec_status;
    pub fn ec_expr_min_max(dt: *const ec_dtype, p: *const *const c_void, masks_or_null: *const *const u8, n_streams: i32,
                           scalars: *const ec_value, n_scalars: i32, steps: *const ec_expr_step, n_steps: i32, n: usize,
                           mn: *mut ec_value, mx: *mut ec_value, s: ec_stream) -> ec_status;
    pub fn ec_expr_min_max_keys(dt: *const ec_dtype, p: *const *const c_void, masks_or_null: *const *const u8, n_streams: i32,
                                scalars: *const ec_value, n_scalars: i32, steps: *const ec_expr_step, n_steps: i32, n: usize,
                                keys2_dev: *mut i64, s: ec_stream) -> ec_status;
    pub fn ec_sharded_expr_min_max(g: *mut ec_shard_group, dt: *const ec_dtype, p: *const *const *const c_void,
                                   masks_or_null: *const *const *const u8, n_streams: i32, scalars: *const ec_value, n_scalars: i32,
                                   steps: *const ec_expr_step, n_steps: i32, n: *const usize, mn: *mut ec_value, mx: *mut ec_value) -> ec_status;
    pub fn ec_expr_source(dt: *const ec_dtype, n_streams: i32, n_scalars: i32, steps: *const ec_expr_step, n_steps: i32,
                          arch_or_null: *const c_char, buf: *mut c_char, cap: usize, len: *mut usize) -> ec_status;
    pub fn ec_host_alloc(hptr: *mut *mut c_void, bytes: usize) -> ec_status;
    pub fn ec_host_free(hptr: *mut c_void) -> ec_status;
    pub fn ec_host_expr(dt: *const ec_dtype, p_host: *const *const c_void, n_streams: i32, scalars: *const ec_value, n_scalars: i32,
                        steps: *const ec_expr_step, n_steps: i32, n: usize, out_host: *mut f64, chunk_cells: usize) -> ec_status;
    pub fn ec_host_masked_expr(dt: *const ec_dtype, p_host: *const *const c_void, nodata: *const *const ec_value, n_streams: i32,
                               scalars: *const ec_value, n_scalars: i32, steps: *const ec_expr_step, n_steps: i32, n: usize,
                               out_host: *mut f64, out_nodata_or_null: *const f64, out_mask_host_or_null: *mut u8, chunk_cells: usize) -> ec_status;
    pub fn ec_comm_get_unique_id(uid: *mut ec_comm_uid) -> ec_status;
    pub fn ec_comm_init_rank(uid: *const ec_comm_uid, n_ranks: i32, rank: i32, comm: *mut ec_comm) -> ec_status;
    pub fn ec_comm_init_all(devices: *const i32, n: i32, comms: *mut ec_comm) -> ec_status;
    pub fn ec_comm_destroy(comm: ec_comm) -> ec_status;
    pub fn ec_allreduce_min_max_keys(comm: ec_comm, keys2_dev: *mut i64, s: ec_stream) -> ec_status;
    pub fn ec_allreduce_counts(comm: ec_comm, counts2_dev: *mut u64, s: ec_stream) -> ec_status;

    pub fn ec_shard_group_create(devices: *const i32, n: i32, flags: u32, out: *mut *mut ec_shard_group) -> ec_status;
    pub fn ec_shard_group_destroy(g: *mut ec_shard_group) -> ec_status;
    pub fn ec_shard_group_size(g: *const ec_shard_group) -> i32;
    pub fn ec_shard_group_shard(g: *const ec_shard_group, shard: i32, device: *mut i32, stream: *mut ec_stream) -> ec_status;
    pub fn ec_shard_group_foreach(g: *mut ec_shard_group, f: ec_shard_fn, user: *mut c_void) -> ec_status;
    pub fn ec_shard_group_sync(g: *mut ec_shard_group) -> ec_status;
    pub fn ec_shard_group_stat(g: *const ec_shard_group, key: *const c_char, value: *mut i64) -> ec_status;
    pub fn ec_sharded_alloc(g: *mut ec_shard_group, bytes: *const usize, dptrs: *mut *mut c_void) -> ec_status;
    pub fn ec_sharded_free(g: *mut ec_shard_group, dptrs: *const *mut c_void) -> ec_status;
    pub fn ec_sharded_upload(g: *mut ec_shard_group, dst_dev: *const *mut c_void, src_host: *const c_void,
                             byte_offsets: *const usize, bytes: *const usize) -> ec_status;
    pub fn ec_sharded_download(g: *mut ec_shard_group, dst_host: *mut c_void, src_dev: *const *const c_void,
                               byte_offsets: *const usize, bytes: *const usize) -> ec_status;
    pub fn ec_sharded_binop(g: *mut ec_shard_group, op: ec_op, lt: ec_dtype, l: *const *const c_void, rt: ec_dtype,
                            r: *const *const c_void, n: *const usize, out: *const *mut f64) -> ec_status;
    pub fn ec_sharded_masked_binop(g: *mut ec_shard_group, op: ec_op, lt: ec_dtype, l: *const *const c_void,
                                   lmask: *const *const u8, rt: ec_dtype, r: *const *const c_void, rmask: *const *const u8,
                                   n: *const usize, out: *const *mut f64, out_mask: *const *mut u8) -> ec_status;
    pub fn ec_sharded_convert(g: *mut ec_shard_group, st: ec_dtype, src: *const *const c_void, dt: ec_dtype,
                              dst: *const *mut c_void, n: *const usize) -> ec_status;
    pub fn ec_sharded_mask_from_nodata(g: *mut ec_shard_group, t: ec_dtype, p: *const *const c_void, n: *const usize,
                                       nd_or_null: *const ec_value, mask: *const *mut u8) -> ec_status;
    pub fn ec_sharded_compare(g: *mut ec_shard_group, rel: i32, lt: ec_dtype, l: *const *const c_void,
                              lmask_or_null: *const *const u8, rt: ec_dtype, r: *const *const c_void,
                              rmask_or_null: *const *const u8, n: *const usize, out_mask: *const *mut u8) -> ec_status;
    pub fn ec_sharded_compare_scalar(g: *mut ec_shard_group, rel: i32, lt: ec_dtype, l: *const *const c_void,
                                     lmask_or_null: *const *const u8, n: *const usize, rhs: *const ec_value,
                                     out_mask: *const *mut u8) -> ec_status;
    pub fn ec_sharded_cast(g: *mut ec_shard_group, mode: i32, st: ec_dtype, src: *const *const c_void, dt: ec_dtype,
                           dst: *const *mut c_void, n: *const usize) -> ec_status;
    pub fn ec_sharded_cast_scaled(g: *mut ec_shard_group, st: ec_dtype, src: *const *const c_void,
                                  masks_or_null: *const *const u8, n: *const usize, scale: f64, offset: f64, dt: ec_dtype,
                                  nodata_or_null: *const ec_value, dst: *const *mut c_void) -> ec_status;
    pub fn ec_sharded_fused(g: *mut ec_shard_group, o1: ec_op, o2: ec_op, o3: ec_op, dt: *const ec_dtype,
                            p: *const *const *const c_void, masks_or_null: *const *const *const u8,
                            scalars_or_null: *const ec_value, n: *const usize, out: *const *mut f64,
                            out_mask_or_null: *const *mut u8) -> ec_status;
    pub fn ec_sharded_expr(g: *mut ec_shard_group, dt: *const ec_dtype, p: *const *const *const c_void,
                           masks_or_null: *const *const *const u8, n_streams: i32, scalars: *const ec_value, n_scalars: i32,
                           steps: *const ec_expr_step, n_steps: i32, n: *const usize, out: *const *mut f64,
                           out_mask_or_null: *const *mut u8) -> ec_status;
    pub fn ec_sharded_host_expr(g: *mut ec_shard_group, dt: *const ec_dtype, p_host: *const *const c_void, nodata_or_null: *const *const ec_value,
                                n_streams: i32, scalars: *const ec_value, n_scalars: i32, steps: *const ec_expr_step, n_steps: i32,
                                n_rows: u64, n_cols: u64, out_host: *mut f64, out_nodata_or_null: *const f64,
                                out_mask_host_or_null: *mut u8, chunk_cells: usize) -> ec_status;
    pub fn ec_sharded_min_max(g: *mut ec_shard_group, t: ec_dtype, p: *const *const c_void,
                              masks_or_null: *const *const u8, n: *const usize, mn: *mut ec_value,
                              mx: *mut ec_value) -> ec_status;
    pub fn ec_sharded_counts(g: *mut ec_shard_group, masks: *const *const u8, n: *const usize, n_true: *mut u64,
                             n_false: *mut u64) -> ec_status;
    // band statistics in one pass (the reference has min_max only, src/buffer.rs:169-173; its NDVI test reads GDAL's
    // STATISTICS_*, src/gdal/rasterband.rs:151-156); the record pointers are `ec_moments` / `ec_stats`, untyped in the header
    pub fn ec_stats_device(t: ec_dtype, p: *const c_void, mask_or_null: *const u8, n: usize, moments_dev: *mut c_void,
                           stream: ec_stream) -> ec_status;
    pub fn ec_stats_fold(moments_host: *const c_void, n_recs: i32, stats_out: *mut c_void) -> ec_status;
    pub fn ec_stats_compute(t: ec_dtype, p: *const c_void, mask_or_null: *const u8, n: usize, stats_out: *mut c_void,
                            stream: ec_stream) -> ec_status;
    pub fn ec_sharded_stats(g: *mut ec_shard_group, t: ec_dtype, p: *const *const c_void,
                            masks_or_null: *const *const u8, n: *const usize, stats_out: *mut c_void) -> ec_status;
    // the band statistics per zone of a zone raster (u8, u16 or i32 ids), and the way back into the raster
    pub fn ec_zonal_workspace_bytes(n_zones: i32) -> usize;
    pub fn ec_zonal_stats_device(t: ec_dtype, p: *const c_void, mask_or_null: *const u8, zt: ec_dtype, zones: *const c_void, n: usize,
                                 n_zones: i32, moments_dev: *mut c_void, workspace_dev: *mut c_void, stream: ec_stream) -> ec_status;
    pub fn ec_zonal_stats_compute(t: ec_dtype, p: *const c_void, mask_or_null: *const u8, zt: ec_dtype, zones: *const c_void, n: usize,
                                  n_zones: i32, stats_out: *mut c_void, stream: ec_stream) -> ec_status;
    pub fn ec_sharded_zonal_stats(g: *mut ec_shard_group, t: ec_dtype, p: *const *const c_void, masks_or_null: *const *const u8,
                                  zt: ec_dtype, zones: *const *const c_void, n: *const usize, n_zones: i32, stats_out: *mut c_void) -> ec_status;
    pub fn ec_zonal_broadcast(zt: ec_dtype, zones: *const c_void, n: usize, n_zones: i32, t: ec_dtype, table_dev: *const c_void,
                              dst: *mut c_void, dst_mask_or_null: *mut u8, stream: ec_stream) -> ec_status;
    // the same records over a per-zone table in global memory: up to EC_ZONAL_TABLE_MAX_ZONES zones, integer atomics only
    pub fn ec_zonal_table_workspace_bytes(t: ec_dtype, n_zones: i32) -> usize;
    pub fn ec_zonal_table_device(t: ec_dtype, p: *const c_void, mask_or_null: *const u8, zt: ec_dtype, zones: *const c_void, n: usize,
                                 n_zones: i32, moments_dev: *mut c_void, workspace_dev: *mut c_void, stream: ec_stream) -> ec_status;
    pub fn ec_zonal_table_compute(t: ec_dtype, p: *const c_void, mask_or_null: *const u8, zt: ec_dtype, zones: *const c_void, n: usize,
                                  n_zones: i32, stats_out: *mut c_void, stream: ec_stream) -> ec_status;
    pub fn ec_sharded_zonal_table(g: *mut ec_shard_group, t: ec_dtype, p: *const *const c_void, masks_or_null: *const *const u8,
                                  zt: ec_dtype, zones: *const *const c_void, n: *const usize, n_zones: i32, stats_out: *mut c_void) -> ec_status;
    pub fn ec_zonal_lookup(zt: ec_dtype, zones: *const c_void, n: usize, n_zones: i32, t: ec_dtype, table_dev: *const c_void,
                           dst: *mut c_void, dst_mask_or_null: *mut u8, stream: ec_stream) -> ec_status;
    // a raster classified by break values: the table built on the host, uploaded by the caller, read by every launch
    pub fn ec_reclass_table_build(t: ec_dtype, bt: ec_dtype, breaks_host: *const c_void, n_breaks: i32, right: i32, dt: ec_dtype,
                                  values: *const ec_value, valid_or_null: *const u8, nodata_or_null: *const ec_value,
                                  table_host_out: *mut c_void) -> ec_status;
    pub fn ec_reclass(t: ec_dtype, src: *const c_void, mask_or_null: *const u8, n: usize, dt: ec_dtype, table_dev: *const c_void,
                      dst: *mut c_void, dst_mask_or_null: *mut u8, stream: ec_stream) -> ec_status;
    pub fn ec_sharded_reclass(g: *mut ec_shard_group, t: ec_dtype, src: *const *const c_void, masks_or_null: *const *const u8,
                              n: *const usize, dt: ec_dtype, tables_dev: *const *const c_void, dst: *const *mut c_void,
                              dst_masks_or_null: *const *mut u8) -> ec_status;
    pub fn ec_shard_range(n_rows: u64, n_cols: u64, shard: u32, n_shards: u32, cell_offset: *mut u64,
                          cell_len: *mut u64) -> ec_status;

    // test support: deterministic device-side inputs and tuning knobs
    // 2-D windows of a resident raster (read_cells(window, window_size, size, e_resample_alg), src/gdal/rasterband.rs:82-125)
    pub fn ec_window(t: ec_dtype, src: *const c_void, src_mask_or_null: *const u8, src_cols: u64, src_rows: u64, x0: u64, y0: u64,
                     win_cols: u64, win_rows: u64, out_cols: u64, out_rows: u64, dst: *mut c_void, dst_mask_or_null: *mut u8,
                     s: ec_stream) -> ec_status;
    pub fn ec_window_resample(alg: i32, t: ec_dtype, src: *const c_void, src_mask_or_null: *const u8, src_cols: u64, src_rows: u64,
                              x0: u64, y0: u64, win_cols: u64, win_rows: u64, out_cols: u64, out_rows: u64, dst: *mut c_void,
                              dst_mask_or_null: *mut u8, s: ec_stream) -> ec_status;
    pub fn ec_focal_result_type(op: i32, t: ec_dtype) -> ec_dtype;
    pub fn ec_focal(op: i32, t: ec_dtype, src: *const c_void, src_mask_or_null: *const u8, cols: u64, rows: u64, rx: u32, ry: u32,
                    flags: u32, dst: *mut c_void, dst_mask_or_null: *mut u8, s: ec_stream) -> ec_status;
    pub fn ec_focal_convolve(t: ec_dtype, src: *const c_void, src_mask_or_null: *const u8, cols: u64, rows: u64,
                             weights_host: *const f64, rx: u32, ry: u32, flags: u32, dst: *mut c_void, dst_mask_or_null: *mut u8,
                             s: ec_stream) -> ec_status;
    pub fn ec_focal_rank(t: ec_dtype, src: *const c_void, src_mask_or_null: *const u8, cols: u64, rows: u64, rx: u32, ry: u32,
                         num: u32, den: u32, method: i32, flags: u32, dst: *mut c_void, dst_mask_or_null: *mut u8,
                         s: ec_stream) -> ec_status;
    pub fn ec_focal_majority(t: ec_dtype, src: *const c_void, src_mask_or_null: *const u8, cols: u64, rows: u64, rx: u32, ry: u32,
                             flags: u32, dst: *mut c_void, dst_mask_or_null: *mut u8, s: ec_stream) -> ec_status;
    // the exact Euclidean distance transform of a mask: squared distances (u32) or distances (f64), or only "within max_sq"
    pub fn ec_distance_workspace_bytes(cols: u64, rows: u64) -> usize;
    pub fn ec_distance(mask: *const u8, cols: u64, rows: u64, max_sq: u32, out_type: ec_dtype, dst_or_null: *mut c_void,
                       dst_mask_or_null: *mut u8, workspace_dev_or_null: *mut c_void, stream: ec_stream) -> ec_status;
    // connected-component labels and the sieve of a raster: i32 labels, validity bytes, the number of kept regions at a device address
    pub fn ec_regions_workspace_bytes(cols: u64, rows: u64) -> usize;
    pub fn ec_regions(t: ec_dtype, src_or_null: *const c_void, src_mask_or_null: *const u8, cols: u64, rows: u64, connectivity: i32,
                      numbering: i32, min_cells: u64, dst_or_null: *mut i32, dst_mask_or_null: *mut u8, n_regions_dev_or_null: *mut u64,
                      workspace_dev_or_null: *mut c_void, stream: ec_stream) -> ec_status;
    pub fn ec_composite_result_type(op: i32, t: ec_dtype) -> ec_dtype;
    pub fn ec_composite(op: i32, t: ec_dtype, layers: *const *const c_void, masks_or_null: *const *const u8, n_layers: i32, n: usize,
                        min_count: u32, dst: *mut c_void, dst_mask_or_null: *mut u8, aux_or_null: *mut u8, s: ec_stream) -> ec_status;
    pub fn ec_sharded_composite(g: *mut ec_shard_group, op: i32, t: ec_dtype, layers: *const *const *const c_void,
                                masks_or_null: *const *const *const u8, n_layers: i32, n: *const usize, min_count: u32,
                                dst: *const *mut c_void, dst_mask_or_null: *const *mut u8, aux_or_null: *const *mut u8) -> ec_status;
    pub fn ec_composite_rank(t: ec_dtype, layers: *const *const c_void, masks_or_null: *const *const u8, n_layers: i32, n: usize,
                             num: u32, den: u32, method: i32, min_count: u32, dst: *mut c_void, dst_mask_or_null: *mut u8,
                             aux_or_null: *mut u8, s: ec_stream) -> ec_status;
    pub fn ec_sharded_composite_rank(g: *mut ec_shard_group, t: ec_dtype, layers: *const *const *const c_void,
                                     masks_or_null: *const *const *const u8, n_layers: i32, n: *const usize, num: u32, den: u32,
                                     method: i32, min_count: u32, dst: *const *mut c_void, dst_mask_or_null: *const *mut u8,
                                     aux_or_null: *const *mut u8) -> ec_status;
    pub fn ec_window_put(t: ec_dtype, tile: *const c_void, tile_mask_or_null: *const u8, win_cols: u64, win_rows: u64,
                         dst: *mut c_void, dst_mask_or_null: *mut u8, dst_cols: u64, dst_rows: u64, x0: u64, y0: u64,
                         s: ec_stream) -> ec_status;

    pub fn ec_synth_fill(t: ec_dtype, dst: *mut c_void, n: usize, seed: u64, base: u64, lo: f64, hi: f64,
                         s: ec_stream) -> ec_status;
    pub fn ec_synth_mask(dst: *mut u8, n: usize, seed: u64, base: u64, pct_nodata: u32, s: ec_stream) -> ec_status;
    pub fn ec_tune_set(key: *const c_char, value: i64) -> ec_status;
    pub fn ec_stat_get(key: *const c_char, value: *mut i64) -> ec_status;
}
