/*
 * erased_cells.h — C ABI of liberased_cells_hip.so: the MI355X (gfx950) drop-in
 * for the per-cell arithmetic path of the Rust crate `erased-cells` 0.1.1.
 *
 * The reference has no FFI seam of its own; the seam is its operator/trait
 * surface.  Each entry point below replaces the BODY of one reference function
 * (cited as path:line relative to the reference tree); the host language keeps
 * the dtype-erased dispatch (`with_ct!`, src/lib.rs:85-101) and the shape rules
 * (zip truncation, empty -> UInt8, length asserts) and calls in here with plain
 * device pointers and sizes.  INTEGRATION.md shows the Rust `extern "C"` block
 * and the operator impls a maintainer would add.
 *
 * Conventions
 *  - Every `const void*` / `void*` data argument is a DEVICE pointer (ec_alloc,
 *    hipMalloc or any other HIP allocation) unless the name says `host`.  It needs
 *    only its cell type's natural alignment: windows at any cell offset are fine.
 *  - Inputs are never written.  Outputs are caller-allocated; the library keeps
 *    no hidden buffers except a small per-stream scratch for reduction partials.
 *  - All compute entry points are asynchronous on `stream` (a hipStream_t; NULL
 *    = the default stream) except those documented as "synchronous result".
 *  - Every function returns ec_status; EC_OK == 0.  No exceptions cross the ABI.
 *    ec_last_error_string() gives the thread-local detail of the last failure.
 *  - dtype codes are `CellType as u8` (src/ctype.rs:11-20, order of
 *    src/lib.rs:89-98): UInt8=0 .. Float64=9.
 *  - Masks are `Vec<bool>` images: one byte per cell, 0 or 1 (src/masked/mask.rs:10-12).
 */
#ifndef ERASED_CELLS_H
#define ERASED_CELLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EC_ABI_VERSION 1

typedef int32_t ec_status;
enum {
    EC_OK = 0,
    EC_ERR_NARROWING = 1,        /* Error::NarrowingError{src,dst}      src/error.rs:14-15 */
    EC_ERR_UNSUPPORTED_TYPE = 2, /* Error::UnsupportedCellTypeError     src/error.rs:16-17 */
    EC_ERR_LENGTH = 3,           /* the reference panics (assert_eq! masked_buffer.rs:48-53) */
    EC_ERR_HIP = 4,              /* a HIP runtime call failed */
    EC_ERR_RCCL = 5,             /* reserved for the collective layer */
    EC_ERR_ARG = 6,              /* null pointer / bad enum */
    EC_ERR_NOT_INITIALIZED = 7
};

/* CellType (src/ctype.rs:11-20). */
typedef uint8_t ec_dtype;
enum {
    EC_U8 = 0, EC_U16 = 1, EC_U32 = 2, EC_U64 = 3,
    EC_I8 = 4, EC_I16 = 5, EC_I32 = 6, EC_I64 = 7,
    EC_F32 = 8, EC_F64 = 9, EC_NTYPES = 10
};

/* Add/Sub/Mul/Div of cb_bin_op! (src/buffer.rs:355-358). */
typedef int32_t ec_op;
enum { EC_ADD = 0, EC_SUB = 1, EC_MUL = 2, EC_DIV = 3 };

/* CellValue (src/value.rs:12-20): tag + payload, 16 bytes. */
typedef struct ec_value {
    uint8_t dtype;
    uint8_t pad_[7];
    union {
        uint8_t u8; uint16_t u16; uint32_t u32; uint64_t u64;
        int8_t i8; int16_t i16; int32_t i32; int64_t i64;
        float f32; double f64;
        uint64_t bits;
    } v;
} ec_value;

typedef void *ec_stream; /* hipStream_t */

/* ---------------------------------------------------------------- *
 * Type lattice — pure host functions, no device needed.
 * ---------------------------------------------------------------- */
ec_dtype ec_union(ec_dtype a, ec_dtype b);          /* CellType::union        src/ctype.rs:99-126  */
int32_t ec_can_fit_into(ec_dtype src, ec_dtype dst); /* CellType::can_fit_into src/ctype.rs:129-131 */
size_t ec_size_of(ec_dtype t);                      /* CellType::size_of      src/ctype.rs:87-96   */
ec_dtype ec_neg_result_type(ec_dtype t);            /* result variant of Neg  src/value.rs:224-240 */
ec_status ec_min_value(ec_dtype t, ec_value *out);  /* CellType::min_value    src/ctype.rs:158-167 */
ec_status ec_max_value(ec_dtype t, ec_value *out);  /* CellType::max_value    src/ctype.rs:170-179 */
/* NoData::<T>::Default.value() (src/masked/nodata.rs:27-38): T::MIN / canonical NaN. */
ec_status ec_nodata_default(ec_dtype t, ec_value *out);
/* CellValue::convert (src/value.rs:74-98) for scalars (host). */
ec_status ec_value_convert(const ec_value *v, ec_dtype dst, ec_value *out);
/* CellValue::to_f64 (src/value.rs:145-156). */
double ec_value_to_f64(const ec_value *v);

/* Row-block sharding: rows [g*R/G, (g+1)*R/G) with the first
 * R mod G shards one row longer; returns the shard's [cell_offset, cell_len). */
ec_status ec_shard_range(uint64_t n_rows, uint64_t n_cols, uint32_t shard, uint32_t n_shards,
                         uint64_t *cell_offset, uint64_t *cell_len);

/* ---------------------------------------------------------------- *
 * Runtime: device, memory, streams, errors.
 * ---------------------------------------------------------------- */
int32_t ec_abi_version(void);
/* The runtime is per device.  ec_init(device) sets up `device` (its CU count, a stream-ordered memory pool the
 * library owns, per-stream reduction scratch) and makes it the calling thread's current library device; it may be
 * called for several devices (one process driving all GPUs of a node) and is idempotent.  Host threads that never
 * chose a device use the first one the process initialised — the one-process-per-GPU shape needs nothing else.
 * ec_set_device switches the calling thread between initialised devices: allocations, streams and launches of a
 * thread go to its current library device.  Device pointers and streams must be used with their own device. */
ec_status ec_init(int32_t device);
ec_status ec_set_device(int32_t device);
ec_status ec_get_device(int32_t *device);
ec_status ec_shutdown(void);         /* waits for every initialised device, frees scratch, trims and destroys the pools */
const char *ec_last_error_string(void);
/* src/dst of the last EC_ERR_NARROWING on this thread (Error::NarrowingError fields). */
ec_status ec_last_narrowing(ec_dtype *src, ec_dtype *dst);
ec_status ec_device_info(int32_t *n_cu, uint64_t *hbm_bytes, char *name, size_t name_cap);

ec_status ec_alloc(void **dptr, size_t bytes);
ec_status ec_free(void *dptr);
/* Stream-ordered allocation from the library's own pool on the current device (hipMallocFromPoolAsync /
 * hipFreeAsync; the device's default pool is never touched): what the host
 * mirrors use for operator results, which the reference allocates per call (`collect()`,
 * src/buffer.rs:327).  A block may be used by work enqueued on `stream` after the call, and freed
 * blocks are recycled without synchronising the device. */
ec_status ec_alloc_async(void **dptr, size_t bytes, ec_stream stream);
/* `stream` must be ordered after the last use of the block (the stream that used it last, normally). */
ec_status ec_free_async(void *dptr, ec_stream stream);
/* Free of a block allocated on `alloc_stream` whose last use was enqueued on `last_use_stream`: the free is queued on
 * `alloc_stream` after an event recorded on `last_use_stream` — what a host mirror's destructor calls, which cannot
 * know on which stream the caller works by the time a buffer is dropped. */
ec_status ec_free_ordered(void *dptr, ec_stream alloc_stream, ec_stream last_use_stream);
/* The pool caches freed blocks up to its release threshold (ec_tune_set("pool_keep_mb"), default 32768 per
 * device); ec_pool_trim waits for the current device and returns everything above `keep_bytes` to the driver. */
ec_status ec_pool_trim(size_t keep_bytes);
ec_status ec_upload(void *dst_dev, const void *src_host, size_t bytes, ec_stream stream);   /* From<Vec<T>> */
ec_status ec_download(void *dst_host, const void *src_dev, size_t bytes, ec_stream stream); /* to_vec; waits for completion */
ec_status ec_copy(void *dst_dev, const void *src_dev, size_t bytes, ec_stream stream);      /* Clone (buffer.rs:151-153) */
ec_status ec_stream_create(ec_stream *out);
/* Allocates the per-stream reduction scratch of a stream the library did not create (NULL = default
 * stream, a torch stream, ...).  After this, every asynchronous entry point — including ec_min_max_keys and
 * ec_mask_counts_device — performs no allocation and no synchronisation (ec_fused over combinations of cell types
 * without a one-pass kernel excepted: it draws temporaries from the stream-ordered pool), so a chain of calls can be captured into a
 * hipGraph on that stream and replayed. */
ec_status ec_prepare_stream(ec_stream stream);
/* Releases that scratch again (the library holds scratch for at most 64 streams per device and recycles the
 * least recently used entry beyond that, so calling this for a dying foreign stream is optional). */
ec_status ec_release_stream(ec_stream stream);
ec_status ec_stream_destroy(ec_stream s);
ec_status ec_stream_sync(ec_stream s);

/* ---------------------------------------------------------------- *
 * Element-wise arithmetic.  out[i] = f64(l[i]) op f64(r[i]), always Float64
 * (src/value.rs:199-217).  `n` = min(len l, len r): the caller applies the zip
 * truncation of src/buffer.rs:327.  n == 0 is a no-op.  Every element-wise entry point of this header writes exactly
 * `n` cells of each of its outputs and no byte in front of or behind them, wherever the output sits (any cell offset:
 * an f64 output at 8 mod 16, a mask at any byte); operands are not written (tests/test_gpu_output_bounds.py).
 * The size one call may cover: the streaming entry points — ec_binop, ec_binop_scalar, ec_masked_binop, ec_neg, ec_convert,
 * ec_fill, ec_fused / ec_masked_fused, ec_expr / ec_masked_expr, the ec_mask_* maps, ec_compare / ec_select, ec_cast /
 * ec_cast_scaled and ec_window's copies — run one workgroup of 256 lanes per tile in ONE launch, and a launch holds at most
 * 2^24 - 1 = 16 777 215 workgroups (a grid's work-items are a 32-bit count).  A call that needs more — 64 GiB or more of one
 * stream: 2^34 cells for a binop or a one-pass tree, 2^37 bytes of a map's widest stream — is refused before any device work:
 * EC_ERR_ARG, nothing written, the message names the limit.  Run it over shards of the buffer.  (The families documented with
 * "more than 2^31 - 1 tiles" — focal, focal_rank, composite, composite_rank, reclass, zonal broadcast, resample — cut a larger job
 * into several launches themselves and keep that limit.)
 * ---------------------------------------------------------------- */
/* impl {Add,Sub,Mul,Div} for &CellBuffer — src/buffer.rs:324-329 */
ec_status ec_binop(ec_op op, ec_dtype lt, const void *l, ec_dtype rt, const void *r,
                   size_t n, double *out, ec_stream stream);
/* impl $trt<R: Into<CellValue>> for CellBuffer — src/buffer.rs:346-352 */
ec_status ec_binop_scalar(ec_op op, ec_dtype lt, const void *l, size_t n, const ec_value *rhs,
                          double *out, ec_stream stream);
/* impl $trt for &MaskedCellBuffer — src/masked/masked_buffer.rs:326-335: the
 * buffer op over ALL cells and `lmask & rmask` (mask.rs:129-140) in one launch. */
ec_status ec_masked_binop(ec_op op, ec_dtype lt, const void *l, const uint8_t *lmask,
                          ec_dtype rt, const void *r, const uint8_t *rmask, size_t n,
                          double *out, uint8_t *out_mask, ec_stream stream);
/* impl Neg for &CellBuffer — src/buffer.rs:360-365 + src/value.rs:224-240.
 * `out` holds n cells of ec_neg_result_type(t). Signed MIN wraps (release build). */
ec_status ec_neg(ec_dtype t, const void *in, size_t n, void *out, ec_stream stream);
/* BufferOps::convert — src/buffer.rs:150-167. EC_ERR_NARROWING iff
 * !can_fit_into(st, dt), decided before any device work; st == dt is a copy. */
ec_status ec_convert(ec_dtype st, const void *src, ec_dtype dt, void *dst, size_t n, ec_stream stream);
/* BufferOps::fill — src/buffer.rs:79-88 (value->dtype must equal t). */
ec_status ec_fill(ec_dtype t, void *dst, size_t n, const ec_value *value, ec_stream stream);

/* Fused two-level expression:  out[i] = (x[i] o1 y[i]) o2 (z[i] o3 w[i])  in one pass,
 * operands dt[k]/p[k] for k = x, y, z, w.  Each step is the same correctly rounded f64 op the eager
 * chain of impl $trt for &CellBuffer (src/buffer.rs:324-329) performs, so the result is bit-identical
 * to evaluating the three operators one by one (e.g. NDVI `(&nir - &red) / (nir + red)`,
 * src/gdal/rasterband.rs:148) while the f64 temporaries never reach HBM.  o3 == EC_OP_NONE: the second
 * term is z alone (`(x o1 y) o2 z`, e.g. `(a + b) * c`) and dt[3]/p[3] are ignored.  Operands may alias.
 * An operand with p[k] == NULL is the scalar `scalars[k]` (the RHS-scalar form of src/buffer.rs:346-352,
 * e.g. `(buf + ones) * 2.0`, examples/masked.rs:12); at least one operand must be a buffer; `n` is the
 * shortest buffer operand's length.  Every call is ONE pass over its operands with no allocation and no
 * synchronisation — whatever the mix of cell types, aliases and scalars — so every call can be captured in a
 * hipGraph: operands of one cell type run a kernel specialised for that type and op triple, every other mix a
 * kernel specialised for the operands' byte widths that widens each cell to f64 in registers (the reference's
 * `unify` + `to_f64`, src/value.rs:103-107,207).  (ec_tune_set("fused_mixed", 0) selects the comparison path of
 * rounds 1-2 instead: convert mixed operands to their CellType::union into pooled temporaries, then fuse.) */
#define EC_OP_NONE (-1)
ec_status ec_fused(ec_op o1, ec_op o2, ec_op o3, const ec_dtype dt[4], const void *const p[4],
                   const ec_value *scalars_or_null, size_t n, double *out, ec_stream stream);
/* The masked form: also out_mask = AND of the buffer operands' masks, as the eager chain of
 * impl $trt for &MaskedCellBuffer (src/masked/masked_buffer.rs:326-364) produces (a scalar has no mask). */
ec_status ec_masked_fused(ec_op o1, ec_op o2, ec_op o3, const ec_dtype dt[4], const void *const p[4],
                          const uint8_t *const masks[4], const ec_value *scalars_or_null, size_t n,
                          double *out, uint8_t *out_mask, ec_stream stream);

/* Expression programs (beyond two levels): a whole operator tree over up to four buffers in ONE pass.
 * The reference evaluates `2.5 * (nir - red) / (nir + 6.0 * red - 7.5 * blue + 1.0)` operator by operator, a pass and an
 * f64 temporary each (impl $trt for &CellBuffer / for CellBuffer with a scalar, src/buffer.rs:324-352); here the same
 * operators run in the same order on registers, every step the same correctly rounded f64 op, so the result is
 * bit-identical to the eager evaluation.  A program is a list of steps `reg[dst] = a op b` over four registers; an
 * operand refers to a stream (buffer k of the call), a register an earlier step wrote, or a scalar; the program's value
 * is what its LAST step computed.  `n` is the shortest buffer's length (zip truncation at every step).  Streams may have
 * any mix of cell types; no allocation, no synchronisation (graph-capturable).  EC_ERR_ARG for a malformed program
 * (bad reference, a register read before it is written, counts out of range). */
typedef struct ec_expr_step {
    int8_t op;  /* EC_ADD .. EC_DIV */
    int8_t a;   /* left operand:  EC_EXPR_STREAM(k) | EC_EXPR_REG(k) | EC_EXPR_SCALAR(k) */
    int8_t b;   /* right operand */
    int8_t dst; /* register 0..3 that receives the result */
} ec_expr_step;
#define EC_EXPR_STREAM(k) ((int8_t)(k))       /* k = 0..3: dt[k] / p[k] of the call */
#define EC_EXPR_REG(k) ((int8_t)(4 + (k)))    /* k = 0..3 */
#define EC_EXPR_SCALAR(k) ((int8_t)(8 + (k))) /* k = 0..7: scalars[k] */
enum { EC_EXPR_MAX_STREAMS = 4, EC_EXPR_REGS = 4, EC_EXPR_MAX_SCALARS = 8, EC_EXPR_MAX_STEPS = 16 };
ec_status ec_expr(const ec_dtype *dt, const void *const *p, int32_t n_streams, const ec_value *scalars,
                  int32_t n_scalars, const ec_expr_step *steps, int32_t n_steps, size_t n, double *out,
                  ec_stream stream);
/* The masked form: also out_mask = AND of the streams' masks, what the eager chain of impl $trt for &MaskedCellBuffer
 * (src/masked/masked_buffer.rs:326-364) leaves behind (scalars carry no mask). */
ec_status ec_masked_expr(const ec_dtype *dt, const void *const *p, const uint8_t *const *masks, int32_t n_streams,
                         const ec_value *scalars, int32_t n_scalars, const ec_expr_step *steps, int32_t n_steps,
                         size_t n, double *out, uint8_t *out_mask, ec_stream stream);
/* BufferOps::min_max (src/buffer.rs:169-173; masked: src/masked/masked_buffer.rs:208-217) of a program's RESULT without
 * its raster: (min, max) under total_cmp of the f64 cells the program computes, over the cells that are valid under the AND
 * of masks_or_null (NULL: all cells), folded from (f64::MAX, f64::MIN) like every min_max here.  Once the program is
 * compiled for itself (below) the streams are read and nothing is written — NDVI's statistics cost the bands' 4 B/cell
 * instead of 4 + 8 + 8; until then (and with expr_jit = 0) the library runs the program into a temporary from its pool and
 * reduces that: two passes, the same answer.  Synchronous. */
ec_status ec_expr_min_max(const ec_dtype *dt, const void *const *p, const uint8_t *const *masks_or_null, int32_t n_streams,
                          const ec_value *scalars, int32_t n_scalars, const ec_expr_step *steps, int32_t n_steps,
                          size_t n, ec_value *mn, ec_value *mx, ec_stream stream);
/* Asynchronous: {~key(min), key(max)} of the same into DEVICE memory keys2_dev, as ec_min_max_keys writes them for a
 * buffer — the 16-byte payload one element-wise MAX all-reduce combines across shards; decode with
 * ec_min_max_decode(EC_F64, ...). */
ec_status ec_expr_min_max_keys(const ec_dtype *dt, const void *const *p, const uint8_t *const *masks_or_null,
                               int32_t n_streams, const ec_value *scalars, int32_t n_scalars, const ec_expr_step *steps,
                               int32_t n_steps, size_t n, int64_t *keys2_dev, ec_stream stream);

/* How ec_expr runs a program.  Three forms, the same cells from each.  (1) Ahead of time: the programs whose TREE is one
 * of NDVI `(a - b) / (a + b)`, `(a + b) * c`, EVI `((a - b) * k0) / (((a + b * k1) - c * k2) + k3)` and `a * k0 + k1`, over
 * distinct streams of one cell width, are built into the library as straight-line kernels (csrc/ec_expr_fixed.hpp) and run
 * that way from their first launch, inside stream captures and without hiprtc; register names, the schedule of independent
 * sub-trees, the numbering of streams and scalars and the side a lone scalar of + or * stands on do not matter
 * (ec_tune_set("expr_fixed", 0) turns this off; ec_stat_get "expr_fixed_launches").  (2) The kernel that serves every
 * other program is an interpreter (a step is decoded once per wave):
 * bound by instruction issue, ≈ 0.04 ms per step over 16384^2 cells beyond the first.  (3) A program is launch-uniform, so
 * the library can also compile it for itself — straight-line code with typed loads, through hiprtc (resolved lazily;
 * without it the interpreter keeps serving) — and cache the module per (program, cell types, load policy).  Same cells
 * either way.  ec_tune_set("expr_jit", v): 0 = never compile; 1 (default) = compile on a background thread once a
 * program has interpreted 2^31 cell-steps, launches interpret until the module is ready; 2 = compile on the calling
 * thread at first sight (≈ 0.3 s per program, 3 s for the first) and fail loudly if that fails.  The environment variable
 * EC_HIPRTC_LIB names the hiprtc library to load instead of libhiprtc.so.  Inside a stream
 * capture a program whose module is not loaded yet is interpreted.  ec_stat_get: "expr_interp_launches",
 * "expr_jit_launches", "expr_jit_compiles", "expr_jit_failures", "expr_jit_programs".
 *
 * ec_expr_source (diagnostics; needs no device): the HIP source the library would compile for the program (every stream
 * non-temporal) into buf[0..cap), *len = bytes needed with the terminating 0; with `arch_or_null` (e.g. "gfx950") also
 * a trial compile, EC_ERR_HIP and the compiler's log in ec_last_error_string() if it fails.  (With the environment
 * variable EC_EXPR_SOURCE_VARIANT=reduce: the variant ec_expr_min_max compiles.) */
ec_status ec_expr_source(const ec_dtype *dt, int32_t n_streams, int32_t n_scalars, const ec_expr_step *steps,
                         int32_t n_steps, const char *arch_or_null, char *buf, size_t cap, size_t *len);

/* Host memory in, host memory out.  The reference's operands and results are Vecs in host memory
 * (src/buffer.rs:12-55, impl $trt for &CellBuffer :324-352); a caller that keeps nothing resident is bound by PCIe —
 * the operands' bytes up, 8 bytes per cell down — not by the kernel.  ec_host_expr evaluates an expression program
 * (ec_expr: a single operator is a one-step program) over HOST arrays p_host[k] of n cells into out_host[0..n): chunks
 * of `chunk_cells` cells (0 = 2^25), upload / kernel / download on three streams over double-buffered device staging
 * (two slots of chunk_cells x (the operands' bytes + 8 [+ masks]) from the library's pool: 2 x 370 MB for u8 / u16 at 2^25),
 * so both directions of the link are busy at once.  Page-locked buffers (ec_host_alloc) are copied asynchronously as
 * they are; any other buffer is page-locked for the duration of the call (hipHostRegister: about one pass over the
 * pages) and, if that is refused, copied through the runtime's pageable path.  Operands may be windows of one array and
 * may overlap each other; out_host may be one of the f64 operands itself (same address), not a shifted window of one.
 * A call that moves at most 64 MiB (and leaves chunk_cells 0) is not worth a pipeline (≈ 1 ms of set-up): it runs as one
 * chunk on the calling thread's own stream (hipStreamPerThread).
 * Synchronous; uses its own streams; may be called from several host threads at once. */
ec_status ec_host_alloc(void **hptr, size_t bytes); /* page-locked host memory */
ec_status ec_host_free(void *hptr);
ec_status ec_host_expr(const ec_dtype *dt, const void *const *p_host, int32_t n_streams, const ec_value *scalars,
                       int32_t n_scalars, const ec_expr_step *steps, int32_t n_steps, size_t n, double *out_host,
                       size_t chunk_cells);
/* The masked form, host to host: MaskedCellBuffer::from_vec_with_nodata (src/masked/masked_buffer.rs:62-71) of every
 * stream — nodata[k] typed as dt[k], or NULL for NoData::None — the program with the AND of the masks (:326-364), and
 * to_vec_with_nodata (:137-152) of the f64 result: out_host[i] = valid ? value : *out_nodata_or_null (NULL: the values of
 * all cells, as the reference computes them); out_mask_host_or_null receives the result's mask (1 = valid).  The masks
 * are derived and applied on the device: what crosses the link is still the operands up and 8 (+ 1) bytes per cell down. */
ec_status ec_host_masked_expr(const ec_dtype *dt, const void *const *p_host, const ec_value *const *nodata,
                              int32_t n_streams, const ec_value *scalars, int32_t n_scalars,
                              const ec_expr_step *steps, int32_t n_steps, size_t n, double *out_host,
                              const double *out_nodata_or_null, uint8_t *out_mask_host_or_null, size_t chunk_cells);

/* ---------------------------------------------------------------- *
 * min/max under the reference's total order (ints natural; floats total_cmp),
 * folded from (T::MAX, T::MIN) — src/buffer.rs:169-173, masked:
 * src/masked/masked_buffer.rs:208-217 (mask may be NULL).
 * ---------------------------------------------------------------- */
/* Synchronous result: waits for the stream, returns host values typed `t`. */
ec_status ec_min_max(ec_dtype t, const void *p, const uint8_t *mask_or_null, size_t n,
                     ec_value *mn, ec_value *mx, ec_stream stream);
/* Asynchronous: writes two order-preserving int64 keys {~key(min), key(max)}
 * to DEVICE memory `keys2_dev`, so that an element-wise MAX all-reduce across
 * shards (RCCL over xGMI) followed by ec_min_max_decode gives the global answer. */
ec_status ec_min_max_keys(ec_dtype t, const void *p, const uint8_t *mask_or_null, size_t n,
                          int64_t *keys2_dev, ec_stream stream);
ec_status ec_min_max_decode(ec_dtype t, const int64_t keys2_host[2], ec_value *mn, ec_value *mx);

/* ---------------------------------------------------------------- *
 * The sharded path: a raster is cut into contiguous row-blocks (ec_shard_range), one per GPU;
 * element-wise kernels are local to a shard, and the only exchange is the all-reduce over xGMI of the
 * 16-byte reduction payloads written by ec_min_max_keys (MAX over two int64) and ec_mask_counts_device
 * (SUM over two uint64).  The reference has no counterpart (it is single-threaded CPU code); what is
 * reduced is BufferOps::min_max (src/buffer.rs:169-173) and Mask::counts (src/masked/mask.rs:72-80).
 * ---------------------------------------------------------------- */
typedef void *ec_comm; /* ncclComm_t; librccl is loaded lazily, EC_ERR_RCCL if it is missing or a call fails */
typedef struct ec_comm_uid { char bytes[128]; } ec_comm_uid; /* ncclUniqueId */
/* One process per GPU: rank 0 makes the id, the host program hands its 128 bytes to the other ranks (a file, a
 * socket, MPI, ...), every rank calls ec_comm_init_rank with its current library device bound (blocks until all
 * n_ranks have joined). */
ec_status ec_comm_get_unique_id(ec_comm_uid *uid);
ec_status ec_comm_init_rank(const ec_comm_uid *uid, int32_t n_ranks, int32_t rank, ec_comm *comm);
/* One process, n GPUs: ec_init()s every listed device and builds the clique (ncclCommInitAll). */
ec_status ec_comm_init_all(const int32_t *devices, int32_t n, ec_comm *comms);
ec_status ec_comm_destroy(ec_comm comm);
/* In-place all-reduce of the device payloads; asynchronous on `stream` (the stream the payload was produced on).
 * (bench.py and the Python mirror use torch.distributed's all_reduce, which is the same RCCL call.) */
ec_status ec_allreduce_min_max_keys(ec_comm comm, int64_t *keys2_dev, ec_stream stream);
ec_status ec_allreduce_counts(ec_comm comm, uint64_t *counts2_dev, ec_stream stream);

/* A shard group: one process driving n GPUs — per device a launch thread bound to it, a stream, a 32-byte payload
 * slot and (unless EC_GROUP_HOST_COMBINE) an RCCL communicator of the n-device clique.  Shard i of every sharded
 * call lives on device i of the group.
 *   Element-wise calls (ec_sharded_binop, _masked_binop, _convert, _mask_from_nodata, _fused) are fire-and-forget:
 * the arguments are checked on the calling thread (EC_ERR_ARG / EC_ERR_UNSUPPORTED_TYPE / EC_ERR_NARROWING come back at
 * once), the per-shard pointer arrays are copied, one job per device is queued for its launch thread, and the call
 * returns without waiting for the launches to be issued: the host can queue the next call while the threads issue
 * this one side by side (host cost per call and per device: profiles/r03/group_fanout.md).  Calls on one group are
 * issued on every device in the order they were made.  A failure inside a queued job (a launch error) is kept by
 * the group and returned — once — by the next ec_shard_group_sync, ec_sharded_min_max or ec_sharded_counts.
 * The device memory named in a call must stay allocated until the group has been synchronised or it is released
 * through ec_sharded_free (which queues behind the launches).  EC_GROUP_BLOCKING_ISSUE restores the form of rounds
 * 1-2: every call waits until all launch threads have issued and returns their first failing status itself.
 *   The reductions return a value and therefore wait; they run in phases (check every shard's arguments, reduce
 * locally on every shard, and only when all of that succeeded exchange the payloads), so a shard that fails cannot
 * leave the others waiting inside a collective.  Should a communicator fail between the ranks' enqueues, the group
 * is poisoned (communicators aborted, every later call EC_ERR_RCCL) rather than left to hang.
 *   EC_GROUP_HOST_COMBINE folds the n 16-byte payloads on the host instead of over xGMI (no RCCL needed; also the
 * only way to list one device twice, e.g. to rehearse on a 1-GPU box). */
typedef struct ec_shard_group ec_shard_group;
enum { EC_GROUP_RCCL = 0, EC_GROUP_HOST_COMBINE = 1, EC_GROUP_BLOCKING_ISSUE = 2 };
ec_status ec_shard_group_create(const int32_t *devices, int32_t n, uint32_t flags, ec_shard_group **out);
ec_status ec_shard_group_destroy(ec_shard_group *g);
int32_t ec_shard_group_size(const ec_shard_group *g);
ec_status ec_shard_group_shard(const ec_shard_group *g, int32_t shard, int32_t *device, ec_stream *stream);
/* Runs fn(shard, device, stream, user) once per shard, each on that shard's launch thread with its device current,
 * concurrently; returns when all have returned (the work they enqueued may still be running): the building block
 * with which a host fans out any entry point of this header.  The first failing status is returned. */
/* (fn must not call ec_shard_group_* / ec_sharded_* of the SAME group — one sharded call runs at a time per group;
 * destroy every group before ec_shutdown().) */
typedef ec_status (*ec_shard_fn)(int32_t shard, int32_t device, ec_stream stream, void *user);
ec_status ec_shard_group_foreach(ec_shard_group *g, ec_shard_fn fn, void *user);
/* Waits until everything queued so far has been issued and every shard's stream has drained; returns (and clears)
 * the first failure a fire-and-forget call left behind. */
ec_status ec_shard_group_sync(ec_shard_group *g);
/* Counters of a group: "jobs_posted" (fire-and-forget jobs queued so far), "poisoned", "blocking_issue". */
ec_status ec_shard_group_stat(const ec_shard_group *g, const char *key, int64_t *value);
/* Per-shard device blocks (bytes[i] on device i) and the scatter / gather of one host buffer by byte ranges
 * (`From<Vec<T>>` / `to_vec` of a sharded buffer; the ranges come from ec_shard_range x sizeof(T)). */
ec_status ec_sharded_alloc(ec_shard_group *g, const size_t *bytes, void **dptrs);
ec_status ec_sharded_free(ec_shard_group *g, void *const *dptrs);
ec_status ec_sharded_upload(ec_shard_group *g, void *const *dst_dev, const void *src_host,
                            const size_t *byte_offsets, const size_t *bytes);
ec_status ec_sharded_download(ec_shard_group *g, void *dst_host, const void *const *src_dev,
                              const size_t *byte_offsets, const size_t *bytes);
/* impl {Add,Sub,Mul,Div} for &CellBuffer (src/buffer.rs:324-329) on every shard; fire-and-forget, no communication. */
ec_status ec_sharded_binop(ec_shard_group *g, ec_op op, ec_dtype lt, const void *const *l, ec_dtype rt,
                           const void *const *r, const size_t *n, double *const *out);
/* The other element-wise entry points on every shard, same arguments as their one-GPU forms with one pointer per
 * shard: impl $trt for &MaskedCellBuffer (src/masked/masked_buffer.rs:326-335), BufferOps::convert
 * (src/buffer.rs:150-167; EC_ERR_NARROWING before any device work), from_vec_with_nodata
 * (src/masked/masked_buffer.rs:62-71), and the fused chains — p[k] is operand k's per-shard pointer array, or NULL
 * for a scalar operand (scalars[k]); masks_or_null / out_mask_or_null both given or both NULL.  Fire-and-forget. */
ec_status ec_sharded_masked_binop(ec_shard_group *g, ec_op op, ec_dtype lt, const void *const *l,
                                  const uint8_t *const *lmask, ec_dtype rt, const void *const *r,
                                  const uint8_t *const *rmask, const size_t *n, double *const *out,
                                  uint8_t *const *out_mask);
ec_status ec_sharded_convert(ec_shard_group *g, ec_dtype st, const void *const *src, ec_dtype dt, void *const *dst,
                             const size_t *n);
ec_status ec_sharded_mask_from_nodata(ec_shard_group *g, ec_dtype t, const void *const *p, const size_t *n,
                                      const ec_value *nd_or_null, uint8_t *const *mask);
ec_status ec_sharded_fused(ec_shard_group *g, ec_op o1, ec_op o2, ec_op o3, const ec_dtype dt[4],
                           const void *const *const p[4], const uint8_t *const *const masks_or_null[4],
                           const ec_value *scalars_or_null, const size_t *n, double *const *out,
                           uint8_t *const *out_mask_or_null);
/* Expression programs (ec_expr / ec_masked_expr) on every shard: p[k] (and masks_or_null[k]) is stream k's per-shard
 * pointer array; masks_or_null / out_mask_or_null both given or both NULL.  A malformed program is EC_ERR_ARG on the
 * calling thread, before anything is posted.  Fire-and-forget. */
ec_status ec_sharded_expr(ec_shard_group *g, const ec_dtype *dt, const void *const *const *p,
                          const uint8_t *const *const *masks_or_null, int32_t n_streams, const ec_value *scalars,
                          int32_t n_scalars, const ec_expr_step *steps, int32_t n_steps, const size_t *n,
                          double *const *out, uint8_t *const *out_mask_or_null);
/* Host memory in, host memory out over all the GPUs of the group: the row-blocks of an n_rows x n_cols raster
 * (ec_shard_range) go through ec_host_expr — or, with nodata_or_null, ec_host_masked_expr — side by side, one pipeline per
 * device: a host-resident raster is then bound by the sum of the GPUs' PCIe links, not by one.  Synchronous. */
ec_status ec_sharded_host_expr(ec_shard_group *g, const ec_dtype *dt, const void *const *p_host,
                               const ec_value *const *nodata_or_null, int32_t n_streams, const ec_value *scalars,
                               int32_t n_scalars, const ec_expr_step *steps, int32_t n_steps, uint64_t n_rows,
                               uint64_t n_cols, double *out_host, const double *out_nodata_or_null,
                               uint8_t *out_mask_host_or_null, size_t chunk_cells);
/* BufferOps::min_max (src/buffer.rs:169-173; masked: src/masked/masked_buffer.rs:208-217) of the whole raster:
 * ec_min_max_keys per shard, one all-reduce(MAX) of the 16-byte keys, decode.  masks_or_null == NULL: unmasked.
 * Synchronous result. */
ec_status ec_sharded_min_max(ec_shard_group *g, ec_dtype t, const void *const *p, const uint8_t *const *masks_or_null,
                             const size_t *n, ec_value *mn, ec_value *mx);
/* min_max of an expression program's result over the whole sharded raster, without the raster: ec_expr_min_max_keys per
 * shard, one all-reduce(MAX) of the 16-byte keys, decode (Float64).  masks_or_null[k]: stream k's per-shard masks.
 * Synchronous result. */
ec_status ec_sharded_expr_min_max(ec_shard_group *g, const ec_dtype *dt, const void *const *const *p,
                                  const uint8_t *const *const *masks_or_null, int32_t n_streams, const ec_value *scalars,
                                  int32_t n_scalars, const ec_expr_step *steps, int32_t n_steps, const size_t *n,
                                  ec_value *mn, ec_value *mx);
/* Mask::counts (src/masked/mask.rs:72-80) of the whole raster: per-shard counts, all-reduce(SUM). Synchronous result. */
ec_status ec_sharded_counts(ec_shard_group *g, const uint8_t *const *masks, const size_t *n,
                            uint64_t *n_true, uint64_t *n_false);

/* ---------------------------------------------------------------- *
 * Ordering / equality of whole buffers, decided on the device (no download of the cells).
 * ---------------------------------------------------------------- */
/* impl Ord / PartialEq for CellBuffer — src/buffer.rs:373-436: cell type first, then the first
 * differing cell under the total order (total_cmp for floats; equality is bit equality), then
 * length.  *ordering = -1 / 0 / +1.  Also serves `Mask` (derived Ord on Vec<bool>, mask.rs:10) with
 * lt == rt == EC_U8.  Synchronous result. */
ec_status ec_buffer_cmp(ec_dtype lt, const void *l, size_t nl, ec_dtype rt, const void *r, size_t nr,
                        int32_t *ordering, ec_stream stream);
/* Index of the first cell whose bits differ in l[0..n) vs r[0..n), or n if none. Synchronous result. */
ec_status ec_first_difference(ec_dtype t, const void *l, const void *r, size_t n, uint64_t *index, ec_stream stream);

/* ---------------------------------------------------------------- *
 * Masks.
 * ---------------------------------------------------------------- */
/* MaskedCellBuffer::from_vec_with_nodata — src/masked/masked_buffer.rs:62-71:
 * mask[i] = !(x[i] == nd) under total-order (bitwise) equality, src/masked/nodata.rs:42-49.
 * nd == NULL is NoData::None (all true). nd->dtype must equal t. */
ec_status ec_mask_from_nodata(ec_dtype t, const void *p, size_t n, const ec_value *nd_or_null,
                              uint8_t *mask, ec_stream stream);
/* MaskedCellBuffer::to_vec_with_nodata — src/masked/masked_buffer.rs:143-151:
 * out[i] = mask[i] ? p[i] : nd ; nd == NULL copies p. */
ec_status ec_mask_select(ec_dtype t, const void *p, const uint8_t *mask, size_t n,
                         const ec_value *nd_or_null, void *out, ec_stream stream);
ec_status ec_mask_and(const uint8_t *l, const uint8_t *r, size_t n, uint8_t *out, ec_stream stream); /* mask.rs:118-140 */
ec_status ec_mask_or(const uint8_t *l, const uint8_t *r, size_t n, uint8_t *out, ec_stream stream);  /* mask.rs:142-163 */
ec_status ec_mask_not(const uint8_t *m, size_t n, uint8_t *out, ec_stream stream);                   /* mask.rs:103-116 */
/* Mask::counts — src/masked/mask.rs:72-80. Synchronous result. */
ec_status ec_mask_counts(const uint8_t *m, size_t n, uint64_t *n_true, uint64_t *n_false, ec_stream stream);
/* Asynchronous: {n_true, n_false} to DEVICE memory (SUM all-reduce across shards). */
ec_status ec_mask_counts_device(const uint8_t *m, size_t n, uint64_t *counts2_dev, ec_stream stream);

/* ---------------------------------------------------------------- *
 * Per-cell order predicates as masks (`ndvi > 0.3`, `qa == 4`, `nir < red`), and the pick of cells by a mask.
 * ---------------------------------------------------------------- */
/* A relation is the truth table over Ordering (impl Ord for CellValue, src/value.rs:248-265): bit 0 = Less, bit 1 = Equal,
 * bit 2 = Greater.  The entry points take it as an int32_t, as every enumeration crosses this ABI (ec_op). */
typedef enum { EC_CMP_LT = 1, EC_CMP_EQ = 2, EC_CMP_LE = 3, EC_CMP_GT = 4, EC_CMP_NE = 5, EC_CMP_GE = 6 } ec_cmp;
/* impl Ord / PartialEq for CellValue — src/value.rs:248-271, cell by cell:
 *   out_mask[i] = (rel >> (1 + CellValue(l[i]).cmp(CellValue(r[i])))) & 1.
 * Both cells are converted to CellType::union(lt, rt) first (`unify`, src/value.rs:103-107), exactly as the reference does: a
 * u64 cell 2^53 + 1 and an i64 cell 2^53 are Equal (their union is Float64), two i64 cells 2^53 and 2^53 + 1 are not.  Integer
 * unions compare naturally, f32 / f64 unions by total_cmp: -0.0 < +0.0, a negative NaN below -inf, a positive NaN above +inf,
 * NaN == NaN for equal bits.  With masks the result is also ANDed with every mask given, in the same launch — the
 * masked-operator rule of src/masked/masked_buffer.rs:326-335: a cell that is not valid satisfies no predicate.  `n` is the caller's zip-truncated length; n == 0 is a no-op.  No allocation, no synchronisation.
 * EC_ERR_ARG (rel outside 1..6, a null pointer with n > 0) and EC_ERR_UNSUPPORTED_TYPE are decided before any device work and
 * without a device.  This family launches at the default "map_u" whatever the knob says. */
ec_status ec_compare(int32_t rel /* an ec_cmp */, ec_dtype lt, const void *l, const uint8_t *lmask_or_null,
                     ec_dtype rt, const void *r, const uint8_t *rmask_or_null,
                     size_t n, uint8_t *out_mask, ec_stream stream);
/* The same with r[i] replaced by the scalar `rhs` (src/value.rs:248-271 with a CellValue on the right); the scalar's own type
 * takes part in the union.  ec_compare_scalar(EC_CMP_NE, t, x, NULL, n, nd) is ec_mask_from_nodata(t, x, n, nd). */
ec_status ec_compare_scalar(int32_t rel /* an ec_cmp */, ec_dtype lt, const void *l, const uint8_t *lmask_or_null,
                            size_t n, const ec_value *rhs, uint8_t *out_mask, ec_stream stream);
/* out[i] = sel[i] ? a[i] : b[i], moved by cell width; a, b and out have type t.  The two-buffer form of
 * to_vec_with_nodata (src/masked/masked_buffer.rs:143-151), where b is a buffer instead of one nodata value: cloud fill,
 * compositing.  out may be a or b (the in-place patch): a lane loads a group of cells before it stores the same group, the
 * reason ec_mask_and may run in place.  Same refusals and guarantees as ec_compare. */
ec_status ec_select(ec_dtype t, const void *a, const void *b, const uint8_t *sel, size_t n,
                    void *out, ec_stream stream);
/* ec_select that also writes out_mask[i] = sel[i] ? amask[i] : bmask[i] (src/masked/masked_buffer.rs:143-151 for two masked
 * buffers).  With sel == amask this is "a where a is valid, else b".  out may be a or b and out_mask
 * amask or bmask, as for ec_select. */
ec_status ec_masked_select(ec_dtype t, const void *a, const uint8_t *amask, const void *b, const uint8_t *bmask,
                           const uint8_t *sel, size_t n, void *out, uint8_t *out_mask, ec_stream stream);
/* ec_compare / ec_compare_scalar on every shard of a group (src/value.rs:248-271 per cell), one pointer per shard as
 * ec_sharded_mask_from_nodata; lmask_or_null / rmask_or_null are NULL or per-shard columns.  Refusals come back on the
 * calling thread before anything is posted.  Fire-and-forget, no communication. */
ec_status ec_sharded_compare(ec_shard_group *g, int32_t rel /* an ec_cmp */, ec_dtype lt, const void *const *l,
                             const uint8_t *const *lmask_or_null, ec_dtype rt, const void *const *r,
                             const uint8_t *const *rmask_or_null, const size_t *n, uint8_t *const *out_mask);
ec_status ec_sharded_compare_scalar(ec_shard_group *g, int32_t rel /* an ec_cmp */, ec_dtype lt, const void *const *l,
                                    const uint8_t *const *lmask_or_null, const size_t *n, const ec_value *rhs,
                                    uint8_t *const *out_mask);

/* ---------------------------------------------------------------- *
 * Results in a storage cell type: f32 rasters, i16 scaled by 10000 with a nodata value, u8 classes.
 * ---------------------------------------------------------------- */
/* How ec_cast turns a cell into a narrower type.  It crosses the ABI as an int32_t, like ec_op and ec_cmp. */
typedef enum { EC_CAST_AS = 0, EC_CAST_ROUND = 1 } ec_cast_mode;
/* dst[i] = src[i] as a cell of type dt, for all 100 type pairs: never EC_ERR_NARROWING (CellValue::convert, src/value.rs:74-98,
 * refuses 59 of them and carries the TODO this answers, src/value.rs:75).
 *   A pair with ec_can_fit_into(st, dt), either mode: exactly ec_convert's cells (and its kernels).
 *   EC_CAST_AS is Rust's `as`: integer to integer keeps the low bits (two's-complement wrap, sign extension); float to integer
 *     truncates toward zero, saturates to dt's range, NaN -> 0; integer to f32 and f64 to f32 round to nearest even, overflow
 *     to +-inf, a NaN stays a NaN of the same sign.
 *   EC_CAST_ROUND is the storing rule: integer to integer is clamped to dt's range, exact in integers (an i64 cell 2^53 + 1
 *     to u64 stays 2^53 + 1); float to integer is trunc(x + copysign(0.5, x)) on the cell widened to f64 — half away from zero
 *     by ONE f64 add, the rule of ec_window_resample — then saturated, the 64-bit limits compared in f64, NaN -> 0; into f32
 *     as EC_CAST_AS.
 * dst must not overlap src.  Asynchronous, no allocation, no synchronisation, capturable; writes exactly n cells of dst, at
 * any cell offset of src and dst.  EC_ERR_ARG (a mode outside {0, 1}, a null pointer with n > 0) and EC_ERR_UNSUPPORTED_TYPE
 * are decided before any device work and without a device; n == 0 is EC_OK and launches nothing.  This family launches at the
 * default "map_u" whatever the knob says. */
ec_status ec_cast(int32_t mode /* an ec_cast_mode */, ec_dtype st, const void *src, ec_dtype dt, void *dst, size_t n,
                  ec_stream stream);
/* The storing direction of a scale and offset (the reading direction is the catalogue program a * k0 + k1):
 *   y = to_f64(src[i]) * scale + offset, the product and the sum rounded individually — never an fma;
 *   dst[i] = y for Float64, EC_CAST_ROUND of y otherwise.
 * With a mask, a cell whose mask byte is 0 receives *nodata_or_null, whatever the cell holds (a NaN leaves no trace):
 * to_vec_with_nodata (src/masked/masked_buffer.rs:137-152) for a type the buffer does not fit into, in one launch.
 * EC_ERR_ARG besides ec_cast's: mask_or_null and nodata_or_null not both given or both NULL, nodata->dtype != dt, scale or
 * offset not finite.  dst must not overlap src or the mask.  Same guarantees as ec_cast. */
ec_status ec_cast_scaled(ec_dtype st, const void *src, const uint8_t *mask_or_null, size_t n,
                         double scale, double offset,
                         ec_dtype dt, const ec_value *nodata_or_null, void *dst, ec_stream stream);
/* ec_cast / ec_cast_scaled on every shard of a group, one pointer per shard as ec_sharded_convert; masks_or_null is NULL or a
 * per-shard column.  Refusals come back on the calling thread before anything is posted.  Fire-and-forget, no communication. */
ec_status ec_sharded_cast(ec_shard_group *g, int32_t mode /* an ec_cast_mode */, ec_dtype st, const void *const *src,
                          ec_dtype dt, void *const *dst, const size_t *n);
ec_status ec_sharded_cast_scaled(ec_shard_group *g, ec_dtype st, const void *const *src,
                                 const uint8_t *const *masks_or_null, const size_t *n, double scale, double offset,
                                 ec_dtype dt, const ec_value *nodata_or_null, void *const *dst);

/* ---------------------------------------------------------------- *
 * 2-D windows of a raster resident on the device.
 * ---------------------------------------------------------------- */
/* RasterBandEx::read_cells / read_cells_masked(window, window_size, size, e_resample_alg) — src/gdal/rasterband.rs:82-125,
 * the part behind the decoder: `src` is a row-major raster of src_cols x src_rows cells of type t on the device; the window
 * of win_cols x win_rows cells at column x0, row y0 is written to `dst` as out_cols x out_rows contiguous cells.
 * out == win copies the cells; any other size resamples by nearest neighbour (GDAL's default; ec_window_resample has the others), defined in
 * integers: output column j reads window column floor((2 j + 1) * win_cols / (2 * out_cols)) — the cell-centre rule
 * (j + 0.5) * win_cols / out_cols evaluated exactly — and rows likewise.  With both masks non-NULL the mask bytes of the same
 * cells move in the same launch (read_cells_masked, rasterband.rs:104-125).  No allocation, asynchronous, capturable.
 * EC_ERR_ARG, before any device work: a window that leaves the raster, src_cols * src_rows or out_cols * out_rows beyond
 * 64 bits, exactly one mask NULL, an empty window with a non-empty output or the reverse, a resampling whose ratio
 * arithmetic leaves 64 bits (an axis of more than 2^31 cells that is neither copied nor reduced by a whole factor).
 * An empty window with an empty output is EC_OK and launches nothing. */
ec_status ec_window(ec_dtype t, const void *src, const uint8_t *src_mask_or_null,
                    uint64_t src_cols, uint64_t src_rows, uint64_t x0, uint64_t y0, uint64_t win_cols, uint64_t win_rows,
                    uint64_t out_cols, uint64_t out_rows, void *dst, uint8_t *dst_mask_or_null, ec_stream stream);
/* The inverse of the copying ec_window (src/gdal/rasterband.rs:82-125 read in the other direction): the contiguous tile of
 * win_cols x win_rows cells is written into the window at (x0, y0) of the raster `dst` of dst_cols x dst_rows cells; no
 * byte outside the window is written.  Same checks, same mask rule. */
ec_status ec_window_put(ec_dtype t, const void *tile, const uint8_t *tile_mask_or_null, uint64_t win_cols, uint64_t win_rows,
                        void *dst, uint8_t *dst_mask_or_null, uint64_t dst_cols, uint64_t dst_rows,
                        uint64_t x0, uint64_t y0, ec_stream stream);
/* The e_resample_alg of read_cells(window, window_size, size, e_resample_alg) — src/gdal/rasterband.rs:37-43, 82-125 — with
 * GDAL's GRIORA_* numbers.  ec_window_resample takes it as an int32_t, as every enumeration crosses this ABI (ec_op). */
typedef enum { EC_RESAMPLE_NEAREST = 0, EC_RESAMPLE_BILINEAR = 1, EC_RESAMPLE_AVERAGE = 5 } ec_resample;
/* An average reduces an axis by at most this factor per call (win <= EC_WINDOW_MAX_REDUCTION * out): a lane walks its
 * footprint in a fixed order, which is what makes the answer unique, and 65 x 65 taps bound its run time.  Chain calls for
 * more, as overview pyramids do. */
enum { EC_WINDOW_MAX_REDUCTION = 64 };
/* ec_window with a resampling algorithm (src/gdal/rasterband.rs:82-125): same arguments and contract after `alg` — no
 * allocation, asynchronous, capturable, output of type t, every check before any device work.  EC_RESAMPLE_NEAREST is
 * ec_window; out == win on both axes is the copy whatever `alg` is; any `alg` but the three above is EC_ERR_ARG naming it
 * (GDAL's Cubic 2, CubicSpline 3, Lanczos 4, Mode 6, Gauss 7 among them).
 * The rule, in integers and individually rounded f64 operations (no FMA), so every cell has one right answer.  Along one
 * axis output index j of `out` over `win` cells has taps (c, w) — window index c, integer weight w > 0 — in ascending order:
 *   AVERAGE   win and out divided by their gcd; lo = j * win, hi = lo + win; c = lo / out .. (hi - 1) / out, w = min((c + 1)
 *             * out, hi) - max(c * out, lo): the overlap with cell c in units of 1 / out cell.  A whole factor is the block mean.
 *   BILINEAR  cell centres, clamped to the WINDOW: t = (2 j + 1) * win + out, k = t / (2 out), f = t % (2 out); taps (k - 1,
 *             2 out - f), (k, f), each index clamped into [0, win - 1], a tap of weight 0 dropped (never read), two taps on
 *             one cell kept as two.
 * Output cell (i, j), ytaps from the row axis, xtaps from the column axis:
 *   acc = 0.0; wsum = 0 (exact, 64 bits)
 *   for (y, wy) in ytaps:  racc = 0.0; rw = 0
 *       for (x, wx) in xtaps:  if no mask or mask[y, x] != 0:  racc = racc + double(wx) * double(cell[y, x]);  rw += wx
 *       acc = acc + double(wy) * racc;  wsum += wy * rw
 *   wsum == 0: value of all-zero bits, out mask 0;  otherwise r = acc / double(wsum), out mask 1
 * f64 takes r, f32 (float)r to nearest even, the integer types trunc(r + copysign(0.5, r)) saturated to the type's range as
 * Rust's `as` does.  double(cell) of a 64-bit integer is the rounding conversion.  A masked-out cell contributes nothing,
 * whatever it holds.
 * EC_ERR_ARG: everything ec_window refuses; an average beyond EC_WINDOW_MAX_REDUCTION on an axis; axis arithmetic beyond
 * 64 bits (win * out for the average, 2 * out * win + out for bilinear); a total weight beyond 64 bits (4 * out_cols *
 * out_rows for bilinear). */
ec_status ec_window_resample(int32_t alg /* an ec_resample */, ec_dtype t, const void *src, const uint8_t *src_mask_or_null,
                             uint64_t src_cols, uint64_t src_rows, uint64_t x0, uint64_t y0,
                             uint64_t win_cols, uint64_t win_rows, uint64_t out_cols, uint64_t out_rows,
                             void *dst, uint8_t *dst_mask_or_null, ec_stream stream);

/* ---------------------------------------------------------------- *
 * Moving windows (focal operations) on a raster resident on the device: every output cell from its neighbours.
 * The reference has no counterpart (its buffers are flat, src/buffer.rs); the 2-D framing is ec_window's: `src` is a
 * row-major raster of cols x rows cells of type t, `dst` one of the same shape, mask bytes move in the same launch.
 * ---------------------------------------------------------------- */
/* What ec_focal computes over a footprint.  It crosses the ABI as an int32_t, like ec_op and ec_resample. */
typedef enum { EC_FOCAL_SUM = 0, EC_FOCAL_MEAN = 1, EC_FOCAL_MIN = 2, EC_FOCAL_MAX = 3 } ec_focal_op;
enum { EC_FOCAL_RADIUS_CAP = 7 };                    /* rx, ry <= 7: footprints up to 15 x 15 */
enum { EC_FOCAL_WHOLE = 1, EC_FOCAL_NORMALIZE = 2 }; /* flags; NORMALIZE is ec_focal_convolve's only */
/* The cell type of ec_focal's result: EC_F64 for SUM and MEAN (the widen-to-f64 rule of the binops), t for MIN and MAX;
 * 255 for an op or a type that is none. */
ec_dtype ec_focal_result_type(int32_t op /* an ec_focal_op */, ec_dtype t);
/* The footprint of output cell (i, j) is the (2 ry + 1) x (2 rx + 1) block of cells around it.  Its TAPS are the cells (y, x)
 * with i - ry <= y <= i + ry and j - rx <= x <= j + rx that lie inside the raster and, when there is a source mask, have
 * mask[y, x] != 0 — taken with rows ascending and columns ascending within a row.  The footprint is clipped at the raster's
 * edges; it never wraps into the neighbouring row.  A cell that is no tap contributes nothing, whatever it holds: a NaN under
 * a cleared mask byte does not reach the result.  The rule, in individually rounded f64 operations (no FMA), so every cell
 * has one right answer:
 *   acc = 0.0; count = 0; [wsum = 0.0]
 *   for y ascending:  racc = 0.0; [rw = 0.0]
 *       for x ascending, (y, x) a tap:
 *           SUM / MEAN  racc = racc + double(cell[y, x])
 *           convolve    racc = racc + (w[y - i + ry, x - j + rx] * double(cell[y, x]));  rw = rw + w[y - i + ry, x - j + rx]
 *           count += 1
 *       acc = acc + racc;  [wsum = wsum + rw]
 *   SUM: r = acc        MEAN: r = acc / double(count)
 *   convolve: r = acc, or with EC_FOCAL_NORMALIZE r = acc / wsum, where wsum == 0.0 counts as "nothing counted"
 *   MIN / MAX: the least / greatest tap under the reference's total order (src/value.rs:248-265, as ec_min_max), its bits copied
 * double(cell) of a 64-bit integer is the rounding conversion, as in ec_window_resample.  (The sum of a single -0.0 is
 * 0.0 + -0.0 = +0.0: the rule, not a copy.)
 * A cell is VALID when count > 0; with EC_FOCAL_WHOLE when count == (2 rx + 1) * (2 ry + 1): every cell of its footprint
 * exists and is unmasked — what a gradient kernel wants at borders and next to holes.  A valid cell stores r and mask byte 1,
 * an invalid one all-zero bits and mask byte 0.  The centre cell's own mask byte has no special role, which is what fills
 * holes from their neighbours; a caller who wants to keep the holes ANDs the result mask with the source mask (ec_mask_and).
 * dst_mask_or_null may be NULL only when src_mask_or_null is NULL and EC_FOCAL_WHOLE is not set; a non-NULL one is always
 * written.  rx == ry == 0 is legal: the widening copy (SUM, MEAN) or the copy (MIN, MAX) with masked-out cells zeroed.
 * dst holds cols * rows cells of ec_focal_result_type(op, t).  No allocation, asynchronous, capturable after
 * ec_prepare_stream.  There is no sharded form: a row-block shard would need ry rows of its neighbour.
 * EC_ERR_ARG, before any device work: a null src or dst, an op that is none, unknown flag bits, EC_FOCAL_NORMALIZE, rx or ry
 * above EC_FOCAL_RADIUS_CAP, dst_mask NULL where it is required, cols * rows beyond 64 bits, more than 2^31 - 1 tiles,
 * dst == src or dst_mask == src_mask.  The operation is not in-place; any other overlap of an output with an input is the
 * caller's to avoid.  A bad dtype is EC_ERR_UNSUPPORTED_TYPE.  cols * rows == 0 is EC_OK and launches nothing. */
ec_status ec_focal(int32_t op /* an ec_focal_op */, ec_dtype t, const void *src, const uint8_t *src_mask_or_null,
                   uint64_t cols, uint64_t rows, uint32_t rx, uint32_t ry, uint32_t flags,
                   void *dst, uint8_t *dst_mask_or_null, ec_stream stream);
/* The weighted form of the rule above (a correlation: weight [dy][dx] meets cell (i - ry + dy, j - rx + dx); flip the
 * weights for a convolution in the strict sense).  weights_host: (2 ry + 1) x (2 rx + 1) doubles, row-major, in HOST memory;
 * they are read before the call returns and travel in the kernel's arguments, so the array has no lifetime requirement and
 * nothing is uploaded.  dst holds cols * rows f64 cells.  With EC_FOCAL_NORMALIZE a cell whose counted weights sum to 0.0 is
 * invalid (zero bits, mask byte 0), also where dst_mask_or_null is NULL.  Same contract and refusals as ec_focal, with a
 * null weights_host among them and EC_FOCAL_NORMALIZE accepted. */
ec_status ec_focal_convolve(ec_dtype t, const void *src, const uint8_t *src_mask_or_null,
                            uint64_t cols, uint64_t rows, const double *weights_host, uint32_t rx, uint32_t ry,
                            uint32_t flags, void *dst /* f64 cells */, uint8_t *dst_mask_or_null, ec_stream stream);

/* Order statistics of a moving window: the median filter, the other window quantiles and the majority (mode) filter.
 * ec_focal's MIN and MAX are the two ends of a footprint's order; ec_focal_rank is any position between them — the median
 * removes a speckle or salt-and-pepper outlier where MEAN smears it and MIN / MAX keep it — and ec_focal_majority is the
 * clean-up step after a classification: every cell takes the class most of its neighbours have.
 * Footprint, TAPS, clipping at the raster's edges (no wrap into the neighbouring row), VALID (count > 0, or
 * count == (2 rx + 1) * (2 ry + 1) under EC_FOCAL_WHOLE), dst_mask_or_null and rx == ry == 0 mean exactly what they mean for
 * ec_focal: a cell that is no tap contributes nothing, whatever it holds; the centre cell's mask byte has no special role; a
 * valid cell stores its result and mask byte 1, an invalid one all-zero bits and mask byte 0.  dst holds cols * rows cells of
 * type t.  No allocation, asynchronous, capturable after ec_prepare_stream, no sharded form.  The only flag is EC_FOCAL_WHOLE.
 * A footprint has at most EC_FOCAL_RANK_MAX_TAPS cells, (2 rx + 1) * (2 ry + 1) <= 64 with rx, ry <= EC_FOCAL_RADIUS_CAP:
 * 3 x 3, 5 x 5, 7 x 7, 7 x 9, 3 x 15, 1 x 15 and so on; 9 x 9 and 15 x 5 are refused.
 * ec_focal_rank, the rule: let c be the number of taps of the cell.  Order the taps ascending by order_key(cell), the
 * reference's total order (src/value.rs:248-265, as ec_min_max and ec_composite_rank use it).  The key is a bijection on
 * bits, so taps of equal key have equal bits and how ties are ordered cannot reach the result.  The position kept is
 * ec_composite_rank's, for q = num / den, 0 <= num <= den, 1 <= den <= EC_RANK_MAX_DEN, counting from 0:
 *   EC_RANK_LOWER   r = (num * (c - 1)) / den
 *   EC_RANK_UPPER   r = (num * (c - 1) + den - 1) / den
 * and the cell stores the bits of the tap at position r.
 *   num = 0 gives the bits and the mask of ec_focal MIN, num = den those of ec_focal MAX.
 *   1/2 LOWER is the lower median, 1/2 UPPER the upper one; they agree where c is odd.
 *   At clipped edges and next to holes r follows the clipped count c, not the footprint's size.
 * ec_focal_majority, the rule: among the taps keep the key that occurs most often; among keys of equal greatest frequency the
 * least under the total order; the cell stores its bits.  "Equal" means equal bits: -0.0 and 0.0 are different keys, and so
 * are NaNs of different payloads.  There is no frequency output and no "strict majority only" flag.
 * Refusals (EC_ERR_ARG, before any device work; a refused call writes nothing), in this order: ec_focal's — a null src or dst,
 * unknown flag bits (every bit but EC_FOCAL_WHOLE), rx or ry above EC_FOCAL_RADIUS_CAP — then more than
 * EC_FOCAL_RANK_MAX_TAPS taps, then ec_focal's again: dst_mask NULL where it is required, cols * rows beyond 64 bits,
 * dst == src or dst_mask == src_mask, more than 2^31 - 1 tiles; for ec_focal_rank then den outside 1 .. EC_RANK_MAX_DEN or
 * num > den, then a method that is none.  A bad dtype is EC_ERR_UNSUPPORTED_TYPE.  cols * rows == 0 is EC_OK and launches
 * nothing. */
enum { EC_FOCAL_RANK_MAX_TAPS = 64 };
ec_status ec_focal_rank(ec_dtype t, const void *src, const uint8_t *src_mask_or_null, uint64_t cols, uint64_t rows,
                        uint32_t rx, uint32_t ry, uint32_t num, uint32_t den, int32_t method /* an ec_rank_method */,
                        uint32_t flags, void *dst, uint8_t *dst_mask_or_null, ec_stream stream);
ec_status ec_focal_majority(ec_dtype t, const void *src, const uint8_t *src_mask_or_null, uint64_t cols, uint64_t rows,
                            uint32_t rx, uint32_t ry, uint32_t flags, void *dst, uint8_t *dst_mask_or_null, ec_stream stream);

/* ---------------------------------------------------------------- *
 * Composites: one raster from a stack of K co-registered layers (dates, tiles, sensors), every output cell from the K cells
 * at its index — the first cloud-free observation, the greatest-value composite, the mean over the clear observations, how
 * many there were, which layer a cell came from.  The reference has no counterpart: its buffers are flat (src/buffer.rs) and
 * its operators take two; the validity rule is its masked one (src/masked/masked_buffer.rs:143-148, 208-217) over K layers.
 * One pass reads every layer once, where a chain of K - 1 ec_masked_select calls re-reads and re-writes the running result.
 * ---------------------------------------------------------------- */
/* What ec_composite keeps of a cell's stack.  It crosses the ABI as an int32_t, like ec_op and ec_focal_op. */
typedef enum { EC_COMPOSITE_FIRST = 0, EC_COMPOSITE_LAST = 1, EC_COMPOSITE_MIN = 2, EC_COMPOSITE_MAX = 3,
               EC_COMPOSITE_SUM = 4, EC_COMPOSITE_MEAN = 5 } ec_composite_op;
enum { EC_COMPOSITE_MAX_LAYERS = 64, EC_COMPOSITE_NONE = 255 };
/* The cell type of ec_composite's result: EC_F64 for SUM and MEAN (the widen-to-f64 rule of the binops), t for the others;
 * 255 for an op or a type that is none. */
ec_dtype ec_composite_result_type(int32_t op /* an ec_composite_op */, ec_dtype t);
/* layers and masks_or_null are HOST arrays of n_layers DEVICE pointers: layer k is n cells of type t at layers[k], with its
 * mask bytes at masks_or_null[k].  masks_or_null == NULL, or an entry masks_or_null[k] == NULL, means every cell of that
 * layer is valid.  Both arrays are read before the call returns and travel in the kernel's arguments, so they have no
 * lifetime requirement and nothing is uploaded.  The same buffer may appear more than once.  A stack of mixed cell types is
 * cast first (ec_cast).
 * The rule, so every cell has one right answer.  Layer k is VALID at cell i when it has no mask or masks[k][i] != 0; count is
 * the number of valid layers at i.  A layer that is not valid contributes nothing, whatever its cell holds: a NaN under a
 * cleared mask byte does not reach the result.
 *   FIRST / LAST  the valid layer with the least / greatest k, its bits copied
 *   MIN / MAX     the least / greatest valid cell under the reference's total order (src/value.rs:248-265, as ec_min_max), its
 *                 bits copied; a layer replaces the running extreme only when it is strictly better, so among cells of equal
 *                 keys the least k wins
 *   SUM           acc = 0.0; for k ascending, layer k valid: acc = acc + double(cell) — every addition one individually
 *                 rounded f64 operation, never an FMA; double(cell) of a 64-bit integer is the rounding conversion, as in
 *                 ec_window_resample.  (The sum of a single -0.0 is 0.0 + -0.0 = +0.0: the rule, not a copy.)
 *   MEAN          acc / double(count)
 * The cell is valid when count >= min_count: it then stores the result and mask byte 1, otherwise all-zero bits and mask
 * byte 0.  1 <= min_count <= n_layers: 1 is the ordinary composite, n_layers the AND rule of the masked operators, a value in
 * between "at least min_count clear observations".
 * aux_or_null is one byte per cell: for FIRST, LAST, MIN and MAX the index k of the layer whose bits were stored, or
 * EC_COMPOSITE_NONE for an invalid cell; for SUM and MEAN count, whether or not the cell is valid.
 * dst holds n cells of ec_composite_result_type(op, t).  dst_mask_or_null may be NULL only when no layer has a mask; a
 * non-NULL one is always written.  No allocation, asynchronous, capturable after ec_prepare_stream.  n == 0 is EC_OK and
 * launches nothing (no pointer is looked at).
 * EC_ERR_ARG, before any device work and in this order: an op that is none; n_layers outside 1 .. EC_COMPOSITE_MAX_LAYERS;
 * min_count outside 1 .. n_layers; (a bad dtype: EC_ERR_UNSUPPORTED_TYPE;) a null layers, layers[k] or dst; dst_mask NULL
 * where it is required; more than 2^31 - 1 tiles; dst equal to a layer; dst_mask or aux equal to a mask, to dst or to each
 * other.  The operation is not in-place; any other overlap of an output with an input is the caller's to avoid.
 * More than 64 layers: compose two calls.  FIRST, LAST, MIN and MAX re-associate over sub-stacks exactly (composite the
 * partial results in stack order, their masks as masks); SUM re-associates up to the rounding of its additions, MEAN from
 * the partial SUMs and counts (aux). */
ec_status ec_composite(int32_t op /* an ec_composite_op */, ec_dtype t, const void *const *layers,
                       const uint8_t *const *masks_or_null, int32_t n_layers, size_t n, uint32_t min_count,
                       void *dst, uint8_t *dst_mask_or_null, uint8_t *aux_or_null, ec_stream stream);
/* ec_composite on every shard of a group (element-wise: no collective).  layers[k] and masks_or_null[k] are columns of one
 * pointer per shard, n the shards' lengths, dst, dst_mask_or_null and aux_or_null columns likewise.  masks_or_null == NULL or
 * masks_or_null[k] == NULL: layer k has no mask on any shard.  The whole-call refusals of ec_composite come first and post
 * nothing. */
ec_status ec_sharded_composite(ec_shard_group *g, int32_t op /* an ec_composite_op */, ec_dtype t,
                               const void *const *const *layers, const uint8_t *const *const *masks_or_null,
                               int32_t n_layers, const size_t *n, uint32_t min_count, void *const *dst,
                               uint8_t *const *dst_mask_or_null, uint8_t *const *aux_or_null);

/* Order statistics of a stack: the median composite and the other quantiles.  ec_composite's MIN and MAX are the two ends of a
 * cell's stack; this is any position between them — the per-cell middle observation of the clear dates survives one unmasked
 * cloud or shadow, where MAX keeps the cloud and MEAN smears it.  The reference has no counterpart (see above).
 * ec_rank_method crosses the ABI as an int32_t, like ec_composite_op. */
typedef enum { EC_RANK_LOWER = 0, EC_RANK_UPPER = 1 } ec_rank_method;
enum { EC_RANK_MAX_DEN = 65535 };
/* layers, masks_or_null, VALID, count, min_count, dst_mask_or_null, aux_or_null and EC_COMPOSITE_NONE mean exactly what they
 * mean for ec_composite; so do n == 0, no allocation, asynchronous, capturable after ec_prepare_stream.  dst holds n cells of
 * type t.  At most EC_COMPOSITE_MAX_LAYERS layers.
 * The rule, so every cell has one right answer.  At cell i let c be the number of valid layers.  Order the valid layers
 * ascending by the pair (order_key(cell), k): the reference's total order (src/value.rs:248-265, as ec_min_max uses it), and
 * among cells of equal key the lesser layer index first.  The pairs are distinct, so the order is total.  The position kept
 * for q = num / den, 0 <= num <= den, 1 <= den <= EC_RANK_MAX_DEN, counting from 0, is
 *   EC_RANK_LOWER   r = (num * (c - 1)) / den
 *   EC_RANK_UPPER   r = (num * (c - 1) + den - 1) / den
 * in integer arithmetic (everything fits 32 bits): numpy.quantile's "lower" / "higher" with an exact rational q.
 * The cell stores the bits of the layer at position r, mask byte 1 and aux = that layer's k iff c >= min_count; otherwise
 * all-zero bits, mask byte 0 and aux = EC_COMPOSITE_NONE.  A layer that is not valid contributes nothing, whatever its cell
 * holds.
 *   1/2 LOWER is the lower median, 1/2 UPPER the upper one; they agree when c is odd.
 *   num = 0 gives the bits and the aux of ec_composite MIN.
 *   num = den gives the bits of ec_composite MAX; its aux is the GREATEST k among cells of equal key, where MAX reports the
 *   least.
 * A mean of the two middles is not built: (lower + upper) / 2 through the operators is the composition.
 * Refusals, before any device work and in this order: n_layers outside 1 .. EC_COMPOSITE_MAX_LAYERS; den outside
 * 1 .. EC_RANK_MAX_DEN or num > den; a method that is none; min_count outside 1 .. n_layers (all EC_ERR_ARG); a bad dtype
 * (EC_ERR_UNSUPPORTED_TYPE); then, for n > 0, ec_composite's pointer, tile-count and aliasing refusals in its order.  A
 * refused call writes nothing. */
ec_status ec_composite_rank(ec_dtype t, const void *const *layers, const uint8_t *const *masks_or_null, int32_t n_layers,
                            size_t n, uint32_t num, uint32_t den, int32_t method /* an ec_rank_method */, uint32_t min_count,
                            void *dst, uint8_t *dst_mask_or_null, uint8_t *aux_or_null, ec_stream stream);
/* ec_composite_rank on every shard of a group, columns as for ec_sharded_composite.  The whole-call refusals of
 * ec_composite_rank come first and post nothing. */
ec_status ec_sharded_composite_rank(ec_shard_group *g, ec_dtype t, const void *const *const *layers,
                                    const uint8_t *const *const *masks_or_null, int32_t n_layers, const size_t *n,
                                    uint32_t num, uint32_t den, int32_t method, uint32_t min_count, void *const *dst,
                                    uint8_t *const *dst_mask_or_null, uint8_t *const *aux_or_null);

/* ---------------------------------------------------------------- *
 * Band statistics: count, min, max, sum, mean and population standard deviation in one pass over a resident buffer.
 * The reference has BufferOps::min_max only (src/buffer.rs:169-173; masked: src/masked/masked_buffer.rs:208-217); its own
 * test of NDVI against GDAL's STATISTICS_MINIMUM / MAXIMUM / MEAN / STDDEV (src/gdal/rasterband.rs:151-156) can therefore
 * assert two of the four.  These entry points compute all of them where the cells are.
 * ---------------------------------------------------------------- */
/* What one launch leaves on the device: 64 bytes.  A cell takes part iff there is no mask or its mask byte is non-zero; a
 * cell that does not contributes nothing, whatever it holds.
 *   kind 0 (u8, i8, u16, i16, u32, i32): exact integers, independent of launch shape, shard cut and order.
 *   kind 1 (u64, i64, f32, f64): cells widened by CellValue::to_f64 (src/value.rs:145-156); pivot c = to_f64(p[0]) if n > 0
 *          and that is finite, else 0.0 — taken whatever the mask says; every counted cell adds d = x - c to s1 and
 *          fma(d, d, s2) to s2.  NaN and infinities propagate by IEEE rules.  No float atomics: the same launch twice gives
 *          the same bits. */
typedef struct ec_moments {
    uint64_t count;    /* cells folded: n, or the mask's true cells */
    int64_t keys2[2];  /* {~key(min), key(max)}, exactly what ec_min_max_keys writes (src/buffer.rs:169-173) */
    int32_t kind;      /* 0: exact integers   1: pivoted f64 */
    int32_t dtype;     /* the ec_dtype scanned */
    union {
        struct { int64_t sum; uint64_t sq_lo, sq_hi; } i; /* sum of x; sum of x * x as a 128-bit unsigned */
        struct { double pivot, s1, s2; } f;               /* c; sum of (x - c); sum of (x - c)^2 */
    } u;
    uint64_t reserved; /* written as 0 */
} ec_moments;
/* min / max as ec_min_max gives them (sentinels (T::MAX, T::MIN) when count == 0); stddev is the population one (divided by
 * count), which is what GDAL's STATISTICS_STDDEV holds (src/gdal/rasterband.rs:151-156); mean = stddev = NaN, sum = 0 when
 * count == 0. */
typedef struct ec_stats {
    uint64_t count;
    ec_value min, max;
    double sum, mean, stddev;
} ec_stats;
/* Record pointers cross the ABI as `void *`, as enumerations cross it as int32_t: `moments_dev` / `moments_host` point at
 * ec_moments, `stats_out` at one ec_stats.
 *
 * ec_stats_device — BufferOps::min_max (src/buffer.rs:169-173; masked: src/masked/masked_buffer.rs:208-217) and the moments
 * of the same cells into the ec_moments at DEVICE address moments_dev.  Asynchronous, no allocation, no synchronisation,
 * capturable (after ec_prepare_stream for a foreign stream).  n == 0 is legal.  EC_ERR_ARG, before any device work: a null
 * pointer, or more cells than the exact sums allow — n > 2^32 for 1- and 2-byte cells, n > 2^31 for u32 / i32 (shard it:
 * these are the bounds under which count * sum(x^2) - sum(x)^2 fits 128 bits in ec_stats_fold). */
ec_status ec_stats_device(ec_dtype t, const void *p, const uint8_t *mask_or_null, size_t n,
                          void *moments_dev, ec_stream stream);
/* Host only, needs no device: folds n_recs ec_moments at HOST address moments_host, left to right, into *stats_out — the
 * STATISTICS_* figures of src/gdal/rasterband.rs:151-156 over all records' cells; min / max as src/buffer.rs:169-173.
 * Every step below is one individually rounded f64 operation (no FMA).  Per record with cnt = count > 0:
 *   kind 0  sum = (double)S1; mean = (double)S1 / (double)cnt; M2 = (double)(cnt * S2 - S1 * S1) / (double)cnt, the
 *           numerator exact in 128 bits;
 *   kind 1  q = s1 / (double)cnt; mean = pivot + q; M2 = s2 - s1 * q, set to 0 if negative (not if NaN);
 *           sum = pivot * (double)cnt + s1.
 * Records with count == 0 are skipped.  Kind-0 records are first added exactly (count, S1, S2), left to right, while the cells
 * they cover stay within one record's limit (ec_stats_device) — so a raster cut into shards folds to the very figures of the
 * raster scanned whole; a run that would pass the limit is closed, enters the merge as one record, and the next begins.
 * What enters the merge (runs, kind-1 records one by one) merges left to right (Chan et al.): n = nA + nB; delta = meanB - meanA;
 * mean = meanA + delta * ((double)nB / (double)n); M2 = (M2A + M2B) + (delta * delta) * ((double)nA * (double)nB / (double)n);
 * sum = sumA + sumB; keys2 by element-wise MAX.  stddev = sqrt(M2 / (double)n).
 * EC_ERR_ARG: a null pointer, n_recs < 1, records of different dtype, a kind that is not its dtype's. */
ec_status ec_stats_fold(const void *moments_host, int32_t n_recs, void *stats_out);
/* ec_stats_device, a 64-byte download, ec_stats_fold: MaskedCellBuffer::min_max (src/masked/masked_buffer.rs:208-217) with
 * the band statistics of src/gdal/rasterband.rs:151-156 beside it.  Synchronous result. */
ec_status ec_stats_compute(ec_dtype t, const void *p, const uint8_t *mask_or_null, size_t n,
                           void *stats_out, ec_stream stream);
/* The same over a sharded raster (BufferOps::min_max, src/buffer.rs:169-173, of the whole): ec_stats_device per shard, the
 * records downloaded and folded on the host in shard order.  No collective, so the result is deterministic and needs no
 * RCCL.  masks_or_null == NULL: unmasked.  Synchronous result. */
ec_status ec_sharded_stats(ec_shard_group *g, ec_dtype t, const void *const *p,
                           const uint8_t *const *masks_or_null, const size_t *n, void *stats_out);

/* ---------------------------------------------------------------- *
 * Zonal statistics: the band statistics above per zone of a zone raster (land-cover classes, regions, basins) in ONE pass
 * over the value raster and the zone raster — "mean NDVI per region" — and the way back into the raster.  The reference has
 * nothing of the kind; the records and the fold are the band statistics' (ec_moments, ec_stats_fold), unchanged.
 *
 * The rule.  zt, the zone raster's cell type, is EC_U8, EC_U16 or EC_I32.  Cell i (i < n) belongs to zone z = zones[i] iff
 * 0 <= z < n_zones and (there is no mask or mask[i] != 0).  A cell with any other id — a negative one, 255 in a u8 class raster
 * used as "outside" — belongs to no zone and contributes nothing, whatever it holds: a NaN under a cleared mask byte or a
 * foreign id reaches no sum.  Record z is the ec_moments that ec_stats_device writes for the cells of zone z:
 *   kind 0  the exact count, sum and sum of squares: independent of launch shape, shard cut and order.
 *   kind 1  s1 = sum of d, s2 = sum of fma(d, d, .), d = to_f64(x) - pivot, with the pivot of the LAUNCH: to_f64(p[0]) if
 *           n > 0 and that is finite, else 0.0 — whatever p[0]'s mask byte or zone is; the same in every record of the call.
 *           No float atomics anywhere: the records are a pure function of the cells, the zones and the launch plan, and the
 *           same call twice gives the same bytes.
 * A zone with no cells gets the empty record (count 0, the sentinels' keys, zero sums, the call's pivot); n == 0 writes
 * n_zones empty records with pivot 0.0.  More than EC_ZONAL_MAX_ZONES zones: ec_zonal_table_* below (up to 2^24 zones; its kind-1
 * sums follow another rule).
 * ---------------------------------------------------------------- */
enum { EC_ZONAL_MAX_ZONES = 256 };
/* Bytes of the workspace ec_zonal_stats_device wants for n_zones zones (a function of n_zones only); 0 for n_zones outside
 * 1 .. EC_ZONAL_MAX_ZONES.  Host only. */
size_t ec_zonal_workspace_bytes(int32_t n_zones);
/* n_zones ec_moments at DEVICE address moments_dev, record z for zone z.  Asynchronous, no allocation, no synchronisation,
 * capturable (after ec_prepare_stream for a foreign stream); the partials go to the caller's workspace_dev
 * (ec_zonal_workspace_bytes(n_zones) bytes, 16-byte aligned, contents scrap afterwards).  Refused before any device work, in
 * this order: n_zones outside 1 .. EC_ZONAL_MAX_ZONES (EC_ERR_ARG); a bad t or zt (EC_ERR_UNSUPPORTED_TYPE); a null pointer
 * (moments_dev, workspace_dev; p and zones unless n == 0); n above ec_stats_device's bound for t; moments_dev or the workspace
 * overlapping an input or each other (all EC_ERR_ARG).  A refused call writes nothing. */
ec_status ec_zonal_stats_device(ec_dtype t, const void *p, const uint8_t *mask_or_null, ec_dtype zt,
                                const void *zones, size_t n, int32_t n_zones, void *moments_dev,
                                void *workspace_dev, ec_stream stream);
/* ec_zonal_stats_device with its workspace from the library's stream-ordered pool, an n_zones x 64-byte download and
 * ec_stats_fold once per zone: n_zones ec_stats at HOST address stats_out.  The same refusals but the workspace's.
 * Synchronous result. */
ec_status ec_zonal_stats_compute(ec_dtype t, const void *p, const uint8_t *mask_or_null, ec_dtype zt,
                                 const void *zones, size_t n, int32_t n_zones, void *stats_out, ec_stream stream);
/* The same over a sharded raster: every shard's n_zones records come down and zone z's records are folded in shard order by
 * ec_stats_fold.  No collective, so kind 0 equals the unsharded figures bit for bit, as ec_sharded_stats promises.
 * masks_or_null == NULL: unmasked.  Synchronous result. */
ec_status ec_sharded_zonal_stats(ec_shard_group *g, ec_dtype t, const void *const *p,
                                 const uint8_t *const *masks_or_null, ec_dtype zt, const void *const *zones,
                                 const size_t *n, int32_t n_zones, void *stats_out);
/* The way back: dst[i] = table[zones[i]] (bits copied) with mask byte 1, for a table of n_zones cells of type t at DEVICE
 * address table_dev — e.g. anomaly = ndvi - the mean of its zone.  A cell whose id belongs to no zone gets all-zero bits and
 * mask byte 0; dst_mask_or_null may be NULL, the zero bits are written all the same.  Element-wise and asynchronous: any n, any
 * cell offset, as the other element-wise entry points; n == 0 is legal.  Refused in the order above: n_zones, a bad t or zt,
 * a null pointer (zones, table_dev, dst), more than 2^31 - 1 tiles, dst or dst_mask overlapping an input or each other.  No
 * sharded form: run it under ec_shard_group_foreach. */
ec_status ec_zonal_broadcast(ec_dtype zt, const void *zones, size_t n, int32_t n_zones, ec_dtype t,
                             const void *table_dev, void *dst, uint8_t *dst_mask_or_null, ec_stream stream);

/* ---------------------------------------------------------------- *
 * Zonal statistics over a table in global memory: the same ec_moments records for up to 2^24 zones — the K labels of ec_regions,
 * a UInt16 parcel raster — where ec_zonal_stats_* stops at EC_ZONAL_MAX_ZONES.  A second family beside the first, which keeps
 * its cap, its refusals and its kind-1 sums; ec_stats_fold and the ec_stats layout are unchanged.
 *
 * Membership is ec_zonal_stats_device's rule unchanged: zt is EC_U8, EC_U16 or EC_I32; cell i belongs to zone z = zones[i] iff
 * 0 <= z < n_zones and (there is no mask or mask[i] != 0); everything else contributes nothing, by a select and never by a
 * multiplication.  n_zones may exceed what zt can hold (the records above the type's range are empty).
 *
 * Record z.  count, keys2, kind, dtype, reserved and the kind-0 sum and 128-bit sq are as ec_zonal_stats_device writes them:
 * exact, independent of launch shape, shard cut and order; for n_zones <= EC_ZONAL_MAX_ZONES the kind-0 records are
 * byte-identical to that call's.  Kind-1 records (u64, i64, f32, f64) DIFFER from that call's in s1 and s2, by construction:
 *   pivot  the call's, as there: to_f64(p[0]) if n > 0 and that is finite, else 0.0, whatever p[0]'s mask byte or zone is.
 *          d = to_f64(x) - pivot, one rounded subtraction.
 *   s1     a truncated fixed-point sum, rounded once, defined per zone.  For the zone's deviations d_1 .. d_m, all finite:
 *          d_j = m_j * 2^-1074 with an integer m_j (exact for every finite f64); L = the bit length of max |m_j|;
 *          k = max(L - 63, 0); t_j = sign(m_j) * (|m_j| >> k) (truncation toward zero, |t_j| < 2^63); T = the exact sum of the
 *          t_j; s1 = T * 2^(k - 1074) rounded to nearest-even f64: +0.0 when T == 0, +-infinity on overflow, as IEEE rounds.
 *   s2     the same rule over w_j = fl(d_j * d_j), one f64 multiply rounded to nearest even (the largest w is fl(dmax * dmax)).
 *          If any w_j is +infinity, s2 = +infinity.
 *   If any d_j is NaN, s1 = s2 = the quiet NaN 0x7FF8000000000000.  Otherwise, with infinities among the d_j: s1 is +infinity or
 *   -infinity for one sign and that NaN for both, s2 = +infinity.  An empty zone has zero sums.
 * What follows: the sums do not depend on order, launch shape, the number of workgroups or how cells are grouped before they
 * are added — permuting the cells of index >= 1 with their zones and mask leaves every byte.  When every d_j is a multiple of the
 * zone's unit 2^(k - 1074) — all data whose deviations span fewer than 63 bits — the sums are the exact sums rounded once.
 * Otherwise |s1 - sum d| < m * 2^(k - 1074) + 1/2 ulp(s1), at least 2^9 times tighter than the (m + 1) u sum|d| bound any order of
 * f64 additions has.  No double rounding at finalize: T * 2^(k - 1074) is a multiple of 2^-1074, and a |T| < 2^53 converts exactly.
 *
 * n.  Kind 0 keeps ec_stats_device's limits.  Kind 1 refuses n > 2^32, which bounds |T| by 2^95.
 *
 * Not here: more than 2^24 zones; UInt32 or 64-bit ids; per-zone medians or histograms; a device-side fold to a table of
 * means (the route back is the host fold, an upload and ec_zonal_lookup); a sharded ec_regions.
 * ---------------------------------------------------------------- */
enum { EC_ZONAL_TABLE_MAX_ZONES = 1 << 24 }; /* a condition, not a measurement: 2^24 records are 1 GiB, and every byte offset
                                              * into the records and the workspace stays below 2^32 */
/* Bytes of the workspace ec_zonal_table_device wants for n_zones zones of values of type t; 0 for a refused n_zones or type.
 * Host only. */
size_t ec_zonal_table_workspace_bytes(ec_dtype t, int32_t n_zones);
/* n_zones ec_moments at DEVICE address moments_dev, record z for zone z.  Asynchronous, no allocation, no synchronisation,
 * capturable (after ec_prepare_stream for a foreign stream); the per-zone table lives in the caller's workspace_dev
 * (ec_zonal_table_workspace_bytes(t, n_zones) bytes, contents scrap afterwards).  n == 0 is legal: n_zones empty records with
 * pivot 0.0.  Refused before any device work and without a device, each with its own text, in this order: n_zones outside
 * 1 .. EC_ZONAL_TABLE_MAX_ZONES (EC_ERR_ARG); a bad t or zt (EC_ERR_UNSUPPORTED_TYPE); a null pointer (moments_dev,
 * workspace_dev; p and zones unless n == 0); n above the kind's bound; moments_dev or workspace_dev not 16-byte aligned, or
 * overlapping an input or each other (all EC_ERR_ARG).  A refused call writes nothing. */
ec_status ec_zonal_table_device(ec_dtype t, const void *p, const uint8_t *mask_or_null, ec_dtype zt,
                                const void *zones, size_t n, int32_t n_zones, void *moments_dev,
                                void *workspace_dev, ec_stream stream);
/* ec_zonal_table_device with its workspace and records from the library's stream-ordered pool, the records' download and
 * ec_stats_fold once per zone: n_zones ec_stats at HOST address stats_out.  The same refusals but the workspace's and the
 * alignment's.  Synchronous result. */
ec_status ec_zonal_table_compute(ec_dtype t, const void *p, const uint8_t *mask_or_null, ec_dtype zt,
                                 const void *zones, size_t n, int32_t n_zones, void *stats_out, ec_stream stream);
/* The same over a sharded raster, columns as ec_sharded_zonal_stats: every shard's n_zones records come down and zone z's
 * records fold in shard order by ec_stats_fold.  No collective: kind 0 equals the unsharded figures bit for bit; each shard's
 * kind-1 record follows the rule above over that shard's cells and pivot.  Synchronous result. */
ec_status ec_sharded_zonal_table(ec_shard_group *g, ec_dtype t, const void *const *p,
                                 const uint8_t *const *masks_or_null, ec_dtype zt, const void *const *zones,
                                 const size_t *n, int32_t n_zones, void *stats_out);
/* ec_zonal_broadcast's rule, word for word, for 1 <= n_zones <= EC_ZONAL_TABLE_MAX_ZONES, with the table read from global
 * memory: dst[i] = table[zones[i]] (bits copied) with mask byte 1; zero bits and mask byte 0 for an id of no zone, also where
 * dst_mask_or_null is NULL.  Element-wise and asynchronous: any n, any cell offset; n == 0 is legal.  Refused as
 * ec_zonal_broadcast refuses, with this family's cap. */
ec_status ec_zonal_lookup(ec_dtype zt, const void *zones, size_t n, int32_t n_zones, ec_dtype t,
                          const void *table_dev, void *dst, uint8_t *dst_mask_or_null, ec_stream stream);

/* ---------------------------------------------------------------- *
 * Reclassification: a raster classified by break values in ONE pass — NDVI into vegetation classes, a DEM into elevation
 * bands, a 16-bit band into a 256-level stretch — where a chain of ec_compare_scalar and ec_select takes a pass per class
 * boundary.  A class raster is a zone raster: ec_reclass then ec_zonal_stats_* is "statistics per class", and its counts are
 * a histogram over any breaks, masked and sharded, in exact integers.  The reference has nothing of the kind; the order is
 * its own (impl Ord for CellValue, src/value.rs:248-265), exactly as ec_compare_scalar decides >=.
 *
 * The rule.  A value raster of cell type t, n_breaks break values b[0 .. n_breaks) of cell type bt (1 <= n_breaks <=
 * EC_RECLASS_MAX_BREAKS), a flag right, n_breaks + 1 class values of the output type dt, an optional validity byte per
 * class, and a nodata value of type dt iff the raster has a mask.
 *   Order    A cell x and a break are compared as ec_compare_scalar compares them: both converted to UT = CellType::union(t, bt)
 *            (`unify`, src/value.rs:103-107) and compared there, integers naturally, f32 / f64 by total_cmp: -0.0 < +0.0, a
 *            negative NaN below -inf, a positive NaN above +inf.  A u64 cell 2^53 + 1 against i64 or f64 breaks compares in
 *            Float64 (it equals a break 2^53); against u64 breaks it compares exactly.
 *   Breaks   strictly ascending in that order after conversion to UT, none a NaN; the builder refuses both.  NaN CELLS are
 *            classified by the total order all the same: with breaks {..., +inf} and right = 1 the top class holds exactly the
 *            positive NaNs; with breaks {-inf, ...} and right = 0 class 0 holds exactly the negative NaNs.
 *   Class    right = 0: c = #{ j : b[j] <= x }, the intervals [b[j-1], b[j]) — numpy.digitize(x, b, right=False);
 *            right = 1: c = #{ j : b[j] <  x }, the intervals (b[j-1], b[j]].  In both 0 <= c <= n_breaks.
 *   Output   no mask or mask[i] != 0: dst[i] = values[c], bits copied, whatever valid[c] says (a class to be dropped gets the
 *            nodata value as its class value).  mask[i] == 0: dst[i] = nodata, whatever the cell holds — a NaN under a cleared
 *            mask byte leaves no trace (the ec_cast_scaled convention).
 *            dst_mask[i] = (mask ? mask[i] != 0 : 1) & (valid ? valid[c] != 0 : 1), written as 0 / 1 iff dst_mask_or_null is
 *            given; it is required when a validity byte is zero (EC_RECLASS_DROPS in the table's flags says so).
 * A pure function of the cells: no tolerance anywhere.
 *
 * The table.  t -> UT is monotone in t's own order and no break is a NaN, so "UT(x) >= b[j]" (right = 1: ">") over the cells
 * of type t is "key(x) >= thr[j]" for ONE threshold in t's order keys (the int64 keys of ec_min_max_keys), found on the host by
 * bisection.  A break no cell of type t reaches (300.0 for a u8 raster) has no threshold; breaks ascend, so these are a suffix:
 * thr[0 .. n_reached) are the thresholds, non-descending (0.2 and 0.7 against an integer raster give the same one; the class
 * between them is empty), and c = #{ j < n_reached : thr[j] <= key(x) }.  The kernels therefore know neither bt nor right.
 * ---------------------------------------------------------------- */
enum { EC_RECLASS_MAX_BREAKS = 255 };     /* up to 256 classes: a UInt8 class raster, EC_ZONAL_MAX_ZONES zones */
enum { EC_RECLASS_HAS_NODATA = 1, EC_RECLASS_DROPS = 2 };  /* ec_reclass_table.flags */
/* What ec_reclass_table_build writes and ec_reclass reads: a fixed-size record with every byte defined (reserved fields, unused
 * thresholds, slots past n_breaks and the high bytes of a value slot are 0), so the same arguments give the same bytes. */
typedef struct ec_reclass_table {
    int32_t t, dt;               /* the raster's and the output's ec_dtype */
    int32_t n_breaks, n_reached; /* 1 .. 255; 0 .. n_breaks */
    uint32_t flags;              /* EC_RECLASS_HAS_NODATA: a nodata value was given (the masked form); EC_RECLASS_DROPS: a
                                    validity byte is zero (a dst_mask is required) */
    uint32_t reserved0;          /* 0 */
    uint64_t nodata_bits;        /* the nodata cell's bytes in the low bytes, or 0 */
    uint64_t reserved1;          /* 0 */
    int64_t thr[255];            /* thr[0 .. n_reached): order keys of t */
    uint64_t value_bits[256];    /* class c's cell of type dt in the low bytes, c <= n_breaks */
    uint8_t valid[256];          /* class c's validity as 0 / 1 (all 1 without validity bytes) */
} ec_reclass_table;
enum { EC_RECLASS_TABLE_BYTES = 4384 };   /* sizeof(ec_reclass_table), a multiple of 16 */
/* Host only, needs no device.  breaks_host: n_breaks cells of type bt; values: n_breaks + 1 ec_value of dtype dt;
 * valid_or_null: n_breaks + 1 bytes; nodata_or_null: given iff the raster has a mask.  Refused in this order: n_breaks outside
 * 1 .. EC_RECLASS_MAX_BREAKS; right outside {0, 1} (EC_ERR_ARG); a bad t, bt or dt (EC_ERR_UNSUPPORTED_TYPE); a null
 * breaks_host, values or table_host_out; a value or the nodata whose dtype is not dt; a NaN break; breaks not strictly
 * ascending in UT (all EC_ERR_ARG).  A refused build writes nothing to table_host_out. */
ec_status ec_reclass_table_build(ec_dtype t, ec_dtype bt, const void *breaks_host, int32_t n_breaks, int32_t right,
                                 ec_dtype dt, const ec_value *values /* n_breaks + 1, each of dtype dt */,
                                 const uint8_t *valid_or_null /* n_breaks + 1 */, const ec_value *nodata_or_null,
                                 void *table_host_out /* EC_RECLASS_TABLE_BYTES */);
/* The rule above over n cells.  table_dev: the built record at a 16-byte-aligned DEVICE address — upload it once (ec_upload)
 * and reuse it across launches, tiles and shards of that device (the table_dev convention of ec_zonal_broadcast).
 * Asynchronous, no allocation, no synchronisation, capturable (after ec_prepare_stream for a foreign stream).  Writes exactly
 * n cells of dst, and n mask bytes when dst_mask_or_null is given, at any cell offset of src, dst and the masks.  n == 0 is
 * EC_OK and launches nothing.  Refused before any device work and without a device, in this order: a bad t or dt
 * (EC_ERR_UNSUPPORTED_TYPE); with n > 0 a null src, table_dev or dst; a table_dev that is not 16-byte aligned; more than
 * 2^31 - 1 tiles; dst or dst_mask overlapping an input, the table or each other (all EC_ERR_ARG; the operation is not in-place).
 * The host cannot read a device record: that the record's t and dt are the call's, and that it was built with a nodata value
 * iff mask_or_null is given, is the caller's to keep — the two calls must agree.  Whatever the record holds, the kernel clamps
 * n_reached to 0 .. 255, reads nothing outside the record's EC_RECLASS_TABLE_BYTES and writes nothing outside dst[0 .. n) and
 * dst_mask[0 .. n). */
ec_status ec_reclass(ec_dtype t, const void *src, const uint8_t *mask_or_null, size_t n,
                     ec_dtype dt, const void *table_dev, void *dst, uint8_t *dst_mask_or_null, ec_stream stream);
/* ec_reclass on every shard of a group (element-wise: no collective, fire-and-forget).  One pointer per shard, as
 * ec_sharded_cast; tables_dev[k] is the record on shard k's device.  masks_or_null / dst_masks_or_null == NULL: none on any
 * shard.  The refusals come back on the calling thread before anything is posted. */
ec_status ec_sharded_reclass(ec_shard_group *g, ec_dtype t, const void *const *src, const uint8_t *const *masks_or_null,
                             const size_t *n, ec_dtype dt, const void *const *tables_dev, void *const *dst,
                             uint8_t *const *dst_masks_or_null);

/* ---------------------------------------------------------------- *
 * Distance: the exact Euclidean distance transform of a mask — "how far is every cell from the nearest cloud / water / road /
 * valid cell" (GDAL's gdal_proximity, scipy.ndimage.distance_transform_edt).  Mask::dilate is a rectangle of at most 15 x 15; this
 * is global, and within(d) is the round buffer.  The reference has nothing of the kind.
 *
 * The rule.  mask is a row-major raster of cols x rows bytes.  Cell (y, x) is a TARGET iff mask[y * cols + x] != 0.  For every
 * cell (i, j):
 *       d2(i, j) = min over targets (y, x) of (i - y)^2 + (j - x)^2          exact integers; 0 on a target
 * The raster does not wrap: distances are between cell indices.  1 <= cols, rows <= EC_DISTANCE_MAX_SIDE, so
 * d2 <= 2 * 32767^2 < 2^31.  A cell is VALID iff at least one target exists and d2 <= max_sq (GDAL's MAXDIST, stated on the
 * squared distance so that it is exact; EC_DISTANCE_UNLIMITED: every cell of a raster with a target).  A valid cell stores, with
 * mask byte 1,
 *       out_type == EC_U32:  d2 as a u32
 *       out_type == EC_F64:  sqrt((double)d2), one correctly rounded IEEE operation
 * and an invalid cell all-zero bits and mask byte 0; the zero bits are written even where dst_mask_or_null is NULL, as
 * ec_zonal_broadcast does.  A pure function of the mask: every cell has one right answer whatever the launch shape.
 *
 * The algorithm is Meijster, Roerdink and Hesselink's (2000), in integers: a sweep down and up every column, then the lower
 * envelope of parabolas along every row.  The workspace holds the column distances (u16) and the row scans' stacks.
 * ---------------------------------------------------------------- */
enum { EC_DISTANCE_MAX_SIDE = 32768 };
#define EC_DISTANCE_UNLIMITED 0xFFFFFFFFu
/* Bytes of the workspace ec_distance wants for a raster of cols x rows cells; 0 for a shape it refuses.  Host only. */
size_t ec_distance_workspace_bytes(uint64_t cols, uint64_t rows);
/* The rule above.  Asynchronous, no synchronisation.  With a workspace of the caller's (ec_distance_workspace_bytes(cols, rows)
 * bytes at a 16-byte-aligned DEVICE address, contents scrap afterwards) there is no allocation and the call is capturable (after
 * ec_prepare_stream for a foreign stream); with workspace_dev_or_null == NULL the workspace comes from the library's
 * stream-ordered pool and goes back to it on the same stream, the way ec_zonal_stats_compute gets its own — still asynchronous.
 * dst_or_null may be NULL when dst_mask_or_null is not: the "within distance" form, in which only the validity bytes are wanted
 * and no value is ever written.  mask and dst_mask may sit at any byte address, dst is aligned to its cell type.  Writes exactly
 * cols * rows cells of dst and cols * rows bytes of dst_mask, each where given.
 * Refused before any device work and without a device, writing nothing, in this order (EC_ERR_ARG unless said otherwise):
 *   1. cols or rows is 0 or above EC_DISTANCE_MAX_SIDE;
 *   2. out_type is neither EC_U32 nor EC_F64: EC_ERR_UNSUPPORTED_TYPE for a value that is no cell type at all, EC_ERR_ARG for a
 *      cell type this entry point does not produce;
 *   3. mask is NULL;
 *   4. dst_or_null and dst_mask_or_null are both NULL;
 *   5. dst is misaligned for out_type;
 *   6. dst, dst_mask or the workspace overlaps mask or each other.
 * There is no sharded form: a row-block shard would need every other shard's columns.  Not here either: anisotropic cells (scale
 * the f64 result), the index of the nearest target, city-block or chessboard metrics, sides above EC_DISTANCE_MAX_SIDE. */
ec_status ec_distance(const uint8_t *mask, uint64_t cols, uint64_t rows, uint32_t max_sq, ec_dtype out_type,
                      void *dst_or_null, uint8_t *dst_mask_or_null, void *workspace_dev_or_null, ec_stream stream);

/* ---------------------------------------------------------------- *
 * Regions: connected-component labels and the sieve of a raster — the contiguous patches of one class, the single clouds, lakes
 * or fields (GDAL's gdal_sieve and gdal_polygonize, GRASS' and terra's clump, scipy.ndimage.label): the step between cleaning a
 * class raster and summarising it by zone.  The reference has nothing of the kind.
 *
 * The rule.  src is a row-major raster of cols x rows cells of cell type t, src_mask_or_null its validity bytes.
 * 1 <= cols, rows <= EC_REGIONS_MAX_SIDE, so n = cols * rows <= 2^30.
 *   Validity.      Cell i is VALID iff there is no mask or mask[i] != 0.
 *   The mask form. With src_or_null == NULL (a mask is then required) every valid cell counts as equal to every other: the
 *                  regions of the mask itself.
 *   Equality.      Otherwise two cells are EQUAL iff their bits are equal — ec_focal_majority's rule, and equality under the total
 *                  order: -0.0 and +0.0 differ, a NaN equals only the same NaN.  Only the cell's WIDTH matters.
 *   Connectivity.  connectivity 4: cells (y, x) and (y', x') are NEIGHBOURS iff |y - y'| + |x - x'| == 1; connectivity 8: iff
 *                  max(|y - y'|, |x - x'|) == 1.  The raster does not wrap: (y, cols - 1) and (y + 1, 0) are not neighbours.
 *   Regions.       Valid cells are CONNECTED iff a chain of neighbouring, valid, pairwise equal cells joins them.  A REGION is a
 *                  maximal connected set, its SIZE its cell count, its ROOT the least row-major index among its cells.
 *   The sieve.     A region is KEPT iff size >= min_cells; 0 and 1 keep everything.
 *   Numbering.     EC_REGIONS_ROOT: the label is root + 1.  EC_REGIONS_DENSE: the kept regions are numbered 1 .. K in increasing
 *                  order of root, dropped regions take no number; for a single class this is scipy.ndimage.label's numbering.
 *   Output.        dst is int32_t labels (EC_I32: a zone raster for ec_zonal_*, label 0 being "no region").  A valid cell of a
 *                  kept region stores its label, with mask byte 1; every other cell all-zero bits and mask byte 0; the zero bits
 *                  are written even where dst_mask_or_null is NULL.  n_regions_dev_or_null, when given, receives K, the number of
 *                  kept regions under either numbering, as a uint64_t at a DEVICE address.  dst_or_null == NULL with a dst_mask
 *                  is the sieve-only form: only the validity bytes are written (what "within" is to ec_distance).
 * A pure function of the inputs: every cell has one right answer whatever the launch shape.
 *
 * The algorithm is the union-find labelling of Komura (2015) and Playne & Hawick (2018): tiles labelled in LDS, their seams
 * joined with atomic minima, the trees flattened, the kept roots counted and numbered by a reduce-then-scan.  The workspace holds
 * a parent and a size per cell (u32 each) and the scan's block sums.
 * ---------------------------------------------------------------- */
enum { EC_REGIONS_MAX_SIDE = 32768 };
typedef enum { EC_REGIONS_ROOT = 0, EC_REGIONS_DENSE = 1 } ec_regions_numbering;
/* Bytes of the workspace ec_regions wants for a raster of cols x rows cells; 0 for a shape it refuses.  Host only. */
size_t ec_regions_workspace_bytes(uint64_t cols, uint64_t rows);
/* The rule above.  Asynchronous, no synchronisation.  With a workspace of the caller's (ec_regions_workspace_bytes(cols, rows)
 * bytes at a 16-byte-aligned DEVICE address, contents scrap afterwards) there is no allocation and the call is capturable (after
 * ec_prepare_stream for a foreign stream); with workspace_dev_or_null == NULL the workspace comes from the library's
 * stream-ordered pool and goes back to it on the same stream, exactly as ec_distance's — still asynchronous.  src_mask and dst_mask
 * may sit at any byte address, src and dst are aligned to their cell type, n_regions_dev_or_null to 8 bytes.  Writes exactly
 * cols * rows cells of dst, cols * rows bytes of dst_mask and the one uint64_t, each where given.
 * Refused before any device work and without a device, writing nothing, each with its own text, in this order (EC_ERR_ARG unless
 * said otherwise):
 *   1. cols or rows is 0 or above EC_REGIONS_MAX_SIDE;
 *   2. t is a bad cell type: EC_ERR_UNSUPPORTED_TYPE; checked only when src_or_null is given;
 *   3. connectivity is neither 4 nor 8;
 *   4. numbering is neither EC_REGIONS_ROOT nor EC_REGIONS_DENSE;
 *   5. src_or_null and src_mask_or_null are both NULL;
 *   6. dst_or_null, dst_mask_or_null and n_regions_dev_or_null are all NULL;
 *   7. src, dst, n_regions_dev_or_null or the workspace is misaligned;
 *   8. an output or the workspace overlaps an input or another output.
 * Not here: a sharded form (a row-block shard needs its neighbours' seams); a per-region size table (the counts of
 * ec_zonal_table_compute over the labels give it, for any K this call can return); merging a dropped region into its largest neighbour (GDAL's sieve does; this one invalidates); sides
 * above EC_REGIONS_MAX_SIDE. */
ec_status ec_regions(ec_dtype t, const void *src_or_null, const uint8_t *src_mask_or_null, uint64_t cols, uint64_t rows,
                     int32_t connectivity, int32_t numbering, uint64_t min_cells,
                     int32_t *dst_or_null, uint8_t *dst_mask_or_null, uint64_t *n_regions_dev_or_null,
                     void *workspace_dev_or_null, ec_stream stream);

/* ---------------------------------------------------------------- *
 * Test/bench support (not part of the reference surface).
 * ---------------------------------------------------------------- */
/* x[i] = lo + splitmix64(seed ^ (base + i)) % (hi - lo + 1), t in {EC_U8, EC_U16, EC_F32}
 * (for EC_F32: uniform on [lo, hi) as float from the same stream). */
ec_status ec_synth_fill(ec_dtype t, void *dst, size_t n, uint64_t seed, uint64_t base,
                        double lo, double hi, ec_stream stream);
/* mask[i] = splitmix64(seed ^ (base+i)) % 100 >= pct_nodata */
ec_status ec_synth_mask(uint8_t *dst, size_t n, uint64_t seed, uint64_t base, uint32_t pct_nodata, ec_stream stream);
/* Tuning knobs (each an atomic word: may be set while other host threads launch).  Accepted values in brackets; a value outside
 * them is SATURATED to the nearer end, or REFUSED (EC_ERR_ARG, the knob unchanged) where so marked; a 0/1 switch stores
 * value != 0.  The value ec_stat_get("tune.<knob>") reads back is the value the launchers act on.
 * "pool_keep_mb" [0, 2^20] (MiB: release threshold of the library's stream-ordered pools); "fused_mixed" 0/1 (1, default:
 * one-pass kernels for fused chains over mixed cell types; 0: convert to the union type first); "binop_variant" {-1, 0, 1},
 * refused otherwise (-1, default: by rule — LDS-staged for an 8-byte operand against one of <= 4 bytes on large rasters; 0 always
 * direct narrow loads; 1 LDS-staged wherever an operand can be staged); "reduce_bpc" [0, 4096] (workgroups per CU for reductions;
 * 0, default: as many as are resident at once); "reduce_shape" {0 .. 4}, refused otherwise (A/B launch shapes of min_max, 0
 * default); "map_u" {1, 2, 4}, refused otherwise (16-B groups per lane per tile of the map kernels); "unaligned_vector" 0/1 (1,
 * default: vector kernels at any cell offset via unaligned global access; 0: pointers that are not 16-byte aligned run the
 * one-cell-per-lane kernels); "peel" {0, 1, 2}, refused otherwise (leading-cell peel of the binop/fused kernels at odd offsets:
 * 0 off, 1 for 1-byte operands (default), 2 also for 2-byte operands).
 * Measurement knobs (defaults are what ships): "mall_mb" [0, 2^20] (MiB); "cache_force" [-1, 255], refused
 * otherwise (-1 off, else the load-policy bits of every launch); "expr_jit" [0, 2]; "expr_fixed" 0/1; "counts_one_launch" [0, 2];
 * and the occupancy caps "write_lds_kb" [0, 64], "binop_lds_kb" [-1, 64], "scalar_lds_kb" [-1, 64], "map_lds_kb" [0, 64],
 * "fused_lds_kb" [0, 64] (KiB of unused LDS reserved per workgroup of a kernel family; -1 = the family's rule).
 * Test hooks (not for production use): "inject_shard_failure" [0, 2^31 - 1], refused otherwise (shard index + 1 whose next job of
 * a shard group fails with EC_ERR_HIP; 0 off); "inject_pin_refusal" 0/1 (1: every host-memory registration is treated as refused). */
ec_status ec_tune_set(const char *key, int64_t value);
/* Counters for tests: "pool_allocs" (ec_alloc_async calls so far, including those the library makes itself — a call
 * that leaves it unchanged allocated nothing), "devices" (initialised devices), "scratch_streams" (streams the
 * library currently holds reduction scratch for), "binop_lds_rule_launches", "expr_fixed_launches", "expr_interp_launches",
 * "expr_jit_launches" (which kernel form a call took); "tune.<knob>": the current value of a knob of ec_tune_set (so that a
 * scope that turns one can put the previous value back). */
ec_status ec_stat_get(const char *key, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* ERASED_CELLS_H */
