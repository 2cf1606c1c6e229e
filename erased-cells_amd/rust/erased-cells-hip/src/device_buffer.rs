//! [`CellBuffer`] with its cells resident in HBM.
//!
//! PROVENANCE.  The type's name, its method signatures and its trait / operator impl headers are the reference's public
//! surface (erased-cells 0.1.1, src/buffer.rs:12-436, MIT License, Copyright (c) 2023 Astraea, Inc.); the bodies are
//! this crate's.  See INTEGRATION.md §2 for the line ranges.
//!
//! The reference's `Vec<T>`-per-variant enum becomes a cell-type tag, a length and one device allocation, and every
//! per-cell iterator chain of the reference becomes one call into liberased_cells_hip.so.  The host keeps what the
//! reference's host code decides once per operation: the dtype tag, zip truncation (the shorter operand wins), and
//! "collecting nothing gives a `UInt8` buffer" (src/buffer.rs:233-234).
use crate::device::{download, stream, upload, DeviceMem};
use crate::error::{check, must, Error, Result};
use crate::ffi::*;
#[cfg(feature = "masked")]
use crate::Mask;
use crate::{with_ct, BufferOps, CellEncoding, CellType, CellValue, Elided};
use num_traits::ToPrimitive;
use std::cmp::Ordering;
use std::fmt::{Debug, Formatter};
use std::ops::{Add, Div, Mul, Neg, Sub};
use std::os::raw::c_void;

/// Cells of one run-time [`CellType`], in HBM.
pub struct CellBuffer {
    pub(crate) ct: CellType,
    pub(crate) len: usize,
    pub(crate) mem: DeviceMem,
}

/// The resampling algorithms of [`CellBuffer::window_resampled`], numbered as GDAL's `GRIORA_*` (`ec_resample`).
#[repr(i32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ResampleAlg {
    NearestNeighbour = EC_RESAMPLE_NEAREST,
    Bilinear = EC_RESAMPLE_BILINEAR,
    Average = EC_RESAMPLE_AVERAGE,
}

/// Band statistics of one pass over a resident buffer (`ec_stats_compute`): `min` / `max` as `min_max()` gives them, `stddev`
/// the population one (divided by `count`), as GDAL's `STATISTICS_STDDEV`.  With `count == 0`: the `(T::MAX, T::MIN)` sentinels,
/// `sum == 0.0`, `mean` and `stddev` NaN.
#[derive(Clone, Copy, Debug)]
pub struct Stats {
    pub count: u64,
    pub min: CellValue,
    pub max: CellValue,
    pub sum: f64,
    pub mean: f64,
    pub stddev: f64,
}

impl Stats {
    pub(crate) fn blank() -> ec_stats {
        let zero = CellValue::UInt8(0).to_ffi();
        ec_stats { count: 0, min: zero, max: zero, sum: 0.0, mean: 0.0, stddev: 0.0 }
    }
    pub(crate) fn from_ffi(s: &ec_stats) -> Self {
        Stats { count: s.count, min: CellValue::from_ffi(&s.min), max: CellValue::from_ffi(&s.max), sum: s.sum, mean: s.mean, stddev: s.stddev }
    }
}

/// A per-cell order predicate (`ec_cmp`): the truth table over `Ordering` — bit 0 `Less`, bit 1 `Equal`, bit 2 `Greater`.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum Cmp {
    Lt = EC_CMP_LT,
    Eq = EC_CMP_EQ,
    Le = EC_CMP_LE,
    Gt = EC_CMP_GT,
    Ne = EC_CMP_NE,
    Ge = EC_CMP_GE,
}

#[cfg(feature = "masked")]
impl CellBuffer {
    /// The [`Mask`] of the cells for which `self[i] rel rhs[i]` holds under `impl Ord for CellValue`, cell by cell: both cells
    /// unified to `CellType::union`, integers natural, floats `total_cmp`.  Zip-truncated; one launch, nothing downloaded.
    /// `lmask` / `rmask`: device bytes ANDed into the result, or null.  The operators `==` `<` `>` of a buffer are not this:
    /// they stay the whole-buffer `Ord`.
    pub(crate) fn compare_raw(&self, rel: Cmp, lmask: *const u8, rhs: &CellBuffer, rmask: *const u8) -> Mask {
        let n = self.len.min(rhs.len);
        let out = Mask::uninit(n);
        must(
            unsafe { ec_compare(rel as i32, self.ct as u8, self.dev_ptr(), lmask, rhs.ct as u8, rhs.dev_ptr(), rmask, n, out.dev_ptr_mut(), stream()) },
            "ec_compare",
        );
        out
    }

    pub(crate) fn compare_scalar_raw(&self, rel: Cmp, lmask: *const u8, rhs: CellValue) -> Mask {
        let out = Mask::uninit(self.len);
        let v = rhs.to_ffi();
        must(
            unsafe { ec_compare_scalar(rel as i32, self.ct as u8, self.dev_ptr(), lmask, self.len, &v, out.dev_ptr_mut(), stream()) },
            "ec_compare_scalar",
        );
        out
    }

    pub fn compare(&self, rel: Cmp, rhs: &CellBuffer) -> Mask {
        self.compare_raw(rel, std::ptr::null(), rhs, std::ptr::null())
    }

    /// [`CellBuffer::compare`] against a scalar; the scalar's own type takes part in the union.
    pub fn compare_scalar<R: Into<CellValue>>(&self, rel: Cmp, rhs: R) -> Mask {
        self.compare_scalar_raw(rel, std::ptr::null(), rhs.into())
    }

    /// `out[i] = mask[i] ? a[i] : b[i]` (`ec_select`), zip-truncated; operands of different cell types meet in their union.
    pub fn select(mask: &Mask, a: &CellBuffer, b: &CellBuffer) -> Result<CellBuffer> {
        if a.ct != b.ct {
            let u = a.ct.union(b.ct);
            return Self::select(mask, &a.convert(u)?, &b.convert(u)?);
        }
        let n = mask.len().min(a.len).min(b.len);
        let out = Self::uninit(a.ct, n);
        check(unsafe { ec_select(a.ct as u8, a.dev_ptr(), b.dev_ptr(), mask.dev_ptr(), n, out.mem.ptr(), stream()) })?;
        Ok(out)
    }
}

/// What [`CellBuffer::focal`] computes over a footprint (`ec_focal_op`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum FocalOp {
    /// The sum of the taps as `Float64`, one partial sum per footprint row.
    Sum = EC_FOCAL_SUM,
    /// The sum divided by the number of taps.
    Mean = EC_FOCAL_MEAN,
    /// The least tap under the total order of `min_max`, its bits copied.
    Min = EC_FOCAL_MIN,
    /// The greatest tap.
    Max = EC_FOCAL_MAX,
}

impl FocalOp {
    /// `Float64` for `Sum` and `Mean` (the widening rule of the operators), `cell_type` for `Min` and `Max`.
    pub fn result_type(self, cell_type: CellType) -> CellType {
        match self {
            FocalOp::Sum | FocalOp::Mean => CellType::Float64,
            FocalOp::Min | FocalOp::Max => cell_type,
        }
    }
}

/// How [`CellBuffer::cast`] turns a cell into a narrower type (`ec_cast_mode`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum CastMode {
    /// Rust's `as`: integers keep their low bits, floats truncate toward zero and saturate, NaN becomes 0.
    As = EC_CAST_AS,
    /// The storing rule: integers are clamped to the range, floats rounded half away from zero and saturated, NaN becomes 0.
    Round = EC_CAST_ROUND,
}

impl CellBuffer {
    /// The cells as type `cell_type`, for every pair of types — where `convert` refuses a narrowing.  A pair that fits is
    /// `convert` in either mode.  One launch.
    pub fn cast(&self, cell_type: CellType, mode: CastMode) -> Result<CellBuffer> {
        let out = Self::uninit(cell_type, self.len);
        check(unsafe { ec_cast(mode as i32, self.ct as u8, self.dev_ptr(), cell_type as u8, out.mem.ptr(), self.len, stream()) })?;
        Ok(out)
    }

    /// `ec_cast_scaled` with a mask and a nodata value of type `cell_type` (both, or a null pointer and `None`).
    pub(crate) fn to_scaled_raw(&self, cell_type: CellType, scale: f64, offset: f64, mask: *const u8, nodata: Option<CellValue>) -> Result<CellBuffer> {
        let out = Self::uninit(cell_type, self.len);
        let marker = nodata.map(|v| v.to_ffi());
        let marker_ptr = marker.as_ref().map_or(std::ptr::null(), |m| m as *const ec_value);
        check(unsafe {
            ec_cast_scaled(self.ct as u8, self.dev_ptr(), mask, self.len, scale, offset, cell_type as u8, marker_ptr, out.mem.ptr(), stream())
        })?;
        Ok(out)
    }

    /// `self * scale + offset` (two rounded f64 steps, never an fma) stored as `cell_type` by the [`CastMode::Round`] rule, in
    /// one launch: `ndvi.to_scaled(CellType::Int16, 10000.0, 0.0)`.
    pub fn to_scaled(&self, cell_type: CellType, scale: f64, offset: f64) -> Result<CellBuffer> {
        self.to_scaled_raw(cell_type, scale, offset, std::ptr::null(), None)
    }
}

impl CellBuffer {
    /// count, min, max, sum, mean and population stddev in one pass over the cells where they are.  `mask`: the device
    /// bytes of a mask of the same length, or null.
    pub(crate) fn stats_raw(&self, mask: *const u8) -> Stats {
        let mut out = Stats::blank();
        must(
            unsafe { ec_stats_compute(self.ct as u8, self.dev_ptr(), mask, self.len, &mut out as *mut ec_stats as *mut c_void, stream()) },
            "ec_stats_compute",
        );
        Stats::from_ffi(&out)
    }

    pub fn stats(&self) -> Stats {
        self.stats_raw(std::ptr::null())
    }

    pub fn new<T: CellEncoding>(data: Vec<T>) -> Self {
        Self::from_host(&data)
    }

    /// `len` cells of type `ct`, contents undefined until a kernel or an upload has written them.
    pub(crate) fn uninit(ct: CellType, len: usize) -> Self {
        CellBuffer { ct, len, mem: DeviceMem::new(len * ct.size_of()) }
    }

    /// The buffer an operator returns when there is nothing to compute.
    pub(crate) fn empty_u8() -> Self {
        Self::uninit(CellType::UInt8, 0)
    }

    pub(crate) fn dev_ptr(&self) -> *const c_void {
        self.mem.ptr()
    }

    /// Device address of cell `index`.
    fn at(&self, index: usize) -> *mut c_void {
        (self.mem.ptr() as usize + index * self.ct.size_of()) as *mut c_void
    }

    fn from_host<T: CellEncoding>(data: &[T]) -> Self {
        let fresh = Self::uninit(T::cell_type(), data.len());
        upload(fresh.mem.ptr(), data);
        fresh
    }

    /// Host copy of cells `[start, start + n)`; `P` must be the buffer's own primitive.
    fn fetch<P: CellEncoding>(&self, start: usize, n: usize) -> Vec<P> {
        assert_eq!(self.ct, P::cell_type(), "a {} buffer holds no {} cells", self.ct, P::cell_type());
        assert!(start + n <= self.len);
        download::<P>(self.at(start), n)
    }

    fn check_index(&self, index: usize) {
        assert!(index < self.len, "index out of bounds: the len is {} but the index is {}", self.len, index);
    }

    /// A copy that is `extra` cells longer (the new cells undefined): the device-side half of `Extend`.
    fn grown_by(&self, extra: usize) -> Self {
        let grown = Self::uninit(self.ct, self.len + extra);
        if self.len > 0 {
            must(unsafe { ec_copy(grown.mem.ptr(), self.dev_ptr(), self.len * self.ct.size_of(), stream()) }, "ec_copy");
        }
        grown
    }

    /// `self op rhs`, cell by cell over the shorter length, always into a Float64 buffer: one `ec_binop` launch.
    pub(crate) fn binop(&self, op: ec_op, rhs: &Self) -> Self {
        let n = usize::min(self.len, rhs.len);
        if n == 0 {
            return Self::empty_u8();
        }
        let result = Self::uninit(CellType::Float64, n);
        must(
            unsafe { ec_binop(op, self.ct as u8, self.dev_ptr(), rhs.ct as u8, rhs.dev_ptr(), n, result.mem.ptr() as *mut f64, stream()) },
            "ec_binop",
        );
        result
    }

    /// `self op scalar`: the scalar crosses the ABI as a tagged value and is widened to f64 once, on the host.
    pub(crate) fn binop_scalar(&self, op: ec_op, rhs: CellValue) -> Self {
        if self.len == 0 {
            return Self::empty_u8();
        }
        let result = Self::uninit(CellType::Float64, self.len);
        let scalar = rhs.to_ffi();
        must(
            unsafe { ec_binop_scalar(op, self.ct as u8, self.dev_ptr(), self.len, &scalar, result.mem.ptr() as *mut f64, stream()) },
            "ec_binop_scalar",
        );
        result
    }

    /// The `window_size` = (w, h) cells at `window` = (x, y) of this buffer read as a raster of rows of `cols` cells, delivered as
    /// `size` = (width, height) cells: the window itself when `size == window_size`, otherwise resampled by nearest neighbour.
    /// One `ec_window` launch; a window that leaves the raster is an error, not a panic.
    pub fn window(&self, cols: usize, window: (usize, usize), window_size: (usize, usize), size: (usize, usize)) -> Result<Self> {
        assert!(if cols == 0 { self.len == 0 } else { self.len % cols == 0 }, "{} cells are not rows of {cols} cells", self.len);
        let rows = if cols == 0 { 0 } else { self.len / cols };
        let cut = Self::uninit(self.ct, size.0 * size.1);
        check(unsafe {
            ec_window(
                self.ct as u8, self.dev_ptr(), std::ptr::null(), cols as u64, rows as u64, window.0 as u64, window.1 as u64,
                window_size.0 as u64, window_size.1 as u64, size.0 as u64, size.1 as u64, cut.mem.ptr(), std::ptr::null_mut(), stream(),
            )
        })?;
        Ok(cut)
    }

    /// [`CellBuffer::window`] with a resampling algorithm: `Bilinear` and `Average` by the rule of `ec_window_resample`
    /// (include/erased_cells.h), `NearestNeighbour` as `window` itself.  One `ec_window_resample` launch; an average that reduces an
    /// axis by more than `EC_WINDOW_MAX_REDUCTION` is an error, chain calls for it.
    pub fn window_resampled(
        &self, cols: usize, window: (usize, usize), window_size: (usize, usize), size: (usize, usize), alg: ResampleAlg,
    ) -> Result<Self> {
        assert!(if cols == 0 { self.len == 0 } else { self.len % cols == 0 }, "{} cells are not rows of {cols} cells", self.len);
        let rows = if cols == 0 { 0 } else { self.len / cols };
        let cut = Self::uninit(self.ct, size.0 * size.1);
        check(unsafe {
            ec_window_resample(
                alg as i32, self.ct as u8, self.dev_ptr(), std::ptr::null(), cols as u64, rows as u64, window.0 as u64, window.1 as u64,
                window_size.0 as u64, window_size.1 as u64, size.0 as u64, size.1 as u64, cut.mem.ptr(), std::ptr::null_mut(), stream(),
            )
        })?;
        Ok(cut)
    }

    /// `ec_focal` with a mask pair (both, or null pointers) and the flags given.
    pub(crate) fn focal_raw(&self, cols: usize, op: FocalOp, radius: (u32, u32), flags: u32, mask: *const u8, out_mask: *mut u8) -> Result<Self> {
        assert!(if cols == 0 { self.len == 0 } else { self.len % cols == 0 }, "{} cells are not rows of {cols} cells", self.len);
        let rows = if cols == 0 { 0 } else { self.len / cols };
        let out = Self::uninit(op.result_type(self.ct), self.len);
        if self.len != 0 {
            check(unsafe {
                ec_focal(op as i32, self.ct as u8, self.dev_ptr(), mask, cols as u64, rows as u64, radius.0, radius.1, flags, out.mem.ptr(), out_mask, stream())
            })?;
        }
        Ok(out)
    }

    /// `ec_focal_convolve`; `weights` is (2 ry + 1) x (2 rx + 1), row-major, read before the call returns.
    pub(crate) fn convolve_raw(&self, cols: usize, weights: &[f64], radius: (u32, u32), flags: u32, mask: *const u8, out_mask: *mut u8) -> Result<Self> {
        assert!(if cols == 0 { self.len == 0 } else { self.len % cols == 0 }, "{} cells are not rows of {cols} cells", self.len);
        assert_eq!(weights.len(), (2 * radius.0 as usize + 1) * (2 * radius.1 as usize + 1), "the weights are not (2 ry + 1) x (2 rx + 1)");
        let rows = if cols == 0 { 0 } else { self.len / cols };
        let out = Self::uninit(CellType::Float64, self.len);
        if self.len != 0 {
            check(unsafe {
                ec_focal_convolve(
                    self.ct as u8, self.dev_ptr(), mask, cols as u64, rows as u64, weights.as_ptr(), radius.0, radius.1, flags, out.mem.ptr(), out_mask,
                    stream(),
                )
            })?;
        }
        Ok(out)
    }

    /// The moving-window `op` over the (2 ry + 1) x (2 rx + 1) footprint of every cell of this buffer read as rows of `cols` cells,
    /// `radius` = (rx, ry), clipped at the raster's edges; the rule is at `ec_focal` in include/erased_cells.h.  One launch.
    pub fn focal(&self, cols: usize, op: FocalOp, radius: (u32, u32)) -> Result<Self> {
        self.focal_raw(cols, op, radius, 0, std::ptr::null(), std::ptr::null_mut())
    }

    /// [`CellBuffer::focal`] where only a cell whose whole footprint lies inside the raster is valid: the cells and the mask that says which.
    pub fn focal_whole(&self, cols: usize, op: FocalOp, radius: (u32, u32)) -> Result<(Self, Mask)> {
        let mask = Mask::uninit(self.len);
        let out = self.focal_raw(cols, op, radius, EC_FOCAL_WHOLE, std::ptr::null(), mask.dev_ptr_mut())?;
        Ok((out, mask))
    }

    /// `ec_focal_rank`, or `ec_focal_majority` when `q` is `None`, with a mask pair (both, or null pointers) and the flags given.
    pub(crate) fn focal_rank_raw(&self, cols: usize, q: Option<(RankFraction, RankMethod)>, radius: (u32, u32), flags: u32, mask: *const u8,
                                 out_mask: *mut u8) -> Result<Self> {
        assert!(if cols == 0 { self.len == 0 } else { self.len % cols == 0 }, "{} cells are not rows of {cols} cells", self.len);
        let rows = if cols == 0 { 0 } else { self.len / cols };
        let out = Self::uninit(self.ct, self.len);
        if self.len != 0 {
            check(unsafe {
                match q {
                    Some((q, method)) => ec_focal_rank(
                        self.ct as u8, self.dev_ptr(), mask, cols as u64, rows as u64, radius.0, radius.1, q.num, q.den, method as i32, flags,
                        out.mem.ptr(), out_mask, stream(),
                    ),
                    None => ec_focal_majority(self.ct as u8, self.dev_ptr(), mask, cols as u64, rows as u64, radius.0, radius.1, flags, out.mem.ptr(), out_mask, stream()),
                }
            })?;
        }
        Ok(out)
    }

    /// The moving-window order statistic: the cells of every footprint (at most `EC_FOCAL_RANK_MAX_TAPS`) in the reference's total
    /// order and the one at position `q * (count - 1)` kept, rounded down or up by `method`; `RankFraction::MEDIAN` is the median
    /// filter, `(0, 1)` [`CellBuffer::focal`] MIN, `(1, 1)` its MAX.  The rule is at `ec_focal_rank` in include/erased_cells.h.  One launch.
    pub fn focal_rank(&self, cols: usize, q: RankFraction, method: RankMethod, radius: (u32, u32)) -> Result<Self> {
        self.focal_rank_raw(cols, Some((q, method)), radius, 0, std::ptr::null(), std::ptr::null_mut())
    }

    /// [`CellBuffer::focal_rank`] at one half: the median filter.  The lower and the upper median agree where the count is odd.
    pub fn focal_median(&self, cols: usize, radius: (u32, u32), method: RankMethod) -> Result<Self> {
        self.focal_rank(cols, RankFraction::MEDIAN, method, radius)
    }

    /// The majority (mode) filter: every cell takes the value most cells of its footprint hold, the least of those that tie under the
    /// total order; "equal" is equal bits.  The rule is at `ec_focal_majority` in include/erased_cells.h.  One launch.
    pub fn focal_majority(&self, cols: usize, radius: (u32, u32)) -> Result<Self> {
        self.focal_rank_raw(cols, None, radius, 0, std::ptr::null(), std::ptr::null_mut())
    }

    /// [`CellBuffer::focal_rank`] where only a cell whose whole footprint lies inside the raster is valid: the cells and the mask that says which.
    pub fn focal_rank_whole(&self, cols: usize, q: RankFraction, method: RankMethod, radius: (u32, u32)) -> Result<(Self, Mask)> {
        let mask = Mask::uninit(self.len);
        let out = self.focal_rank_raw(cols, Some((q, method)), radius, EC_FOCAL_WHOLE, std::ptr::null(), mask.dev_ptr_mut())?;
        Ok((out, mask))
    }

    /// [`CellBuffer::focal_majority`] where only a cell whose whole footprint lies inside the raster is valid.
    pub fn focal_majority_whole(&self, cols: usize, radius: (u32, u32)) -> Result<(Self, Mask)> {
        let mask = Mask::uninit(self.len);
        let out = self.focal_rank_raw(cols, None, radius, EC_FOCAL_WHOLE, std::ptr::null(), mask.dev_ptr_mut())?;
        Ok((out, mask))
    }

    /// The weighted moving-window sum (a correlation: weight `[dy][dx]` meets cell `(i - ry + dy, j - rx + dx)`) as `Float64` cells;
    /// `normalize` divides by the sum of the weights counted.  One launch; the weights travel in the kernel's arguments.
    pub fn convolve(&self, cols: usize, weights: &[f64], radius: (u32, u32), normalize: bool) -> Result<Self> {
        let flags = if normalize { EC_FOCAL_NORMALIZE } else { 0 };
        self.convolve_raw(cols, weights, radius, flags, std::ptr::null(), std::ptr::null_mut())
    }

    /// [`CellBuffer::convolve`] where only a cell whose whole footprint lies inside the raster is valid — what a gradient kernel wants
    /// at the borders: the cells and the mask that says which.
    pub fn convolve_whole(&self, cols: usize, weights: &[f64], radius: (u32, u32), normalize: bool) -> Result<(Self, Mask)> {
        let mask = Mask::uninit(self.len);
        let flags = EC_FOCAL_WHOLE | if normalize { EC_FOCAL_NORMALIZE } else { 0 };
        let out = self.convolve_raw(cols, weights, radius, flags, std::ptr::null(), mask.dev_ptr_mut())?;
        Ok((out, mask))
    }

    /// Writes `tile` (`window_size` = (w, h) contiguous cells of this buffer's cell type) into the window at `window` = (x, y)
    /// of this buffer read as rows of `cols` cells; no cell outside the window changes.  One `ec_window_put` launch.
    pub fn put_window(&mut self, cols: usize, window: (usize, usize), window_size: (usize, usize), tile: &Self) -> Result<()> {
        assert!(if cols == 0 { self.len == 0 } else { self.len % cols == 0 }, "{} cells are not rows of {cols} cells", self.len);
        assert_eq!(self.ct, tile.ct, "a {} tile does not go into a {} buffer", tile.ct, self.ct);
        assert_eq!(tile.len, window_size.0 * window_size.1, "the tile is not {} x {} cells", window_size.0, window_size.1);
        let rows = if cols == 0 { 0 } else { self.len / cols };
        check(unsafe {
            ec_window_put(
                self.ct as u8, tile.dev_ptr(), std::ptr::null(), window_size.0 as u64, window_size.1 as u64, self.mem.ptr(),
                std::ptr::null_mut(), cols as u64, rows as u64, window.0 as u64, window.1 as u64, stream(),
            )
        })
    }

    /// `-self`, in the cell type the reference's scalar negation produces (`ec_neg_result_type`).
    fn negated(&self) -> Self {
        if self.len == 0 {
            return Self::empty_u8();
        }
        let result = Self::uninit(CellType::from_code(unsafe { ec_neg_result_type(self.ct as u8) }), self.len);
        must(unsafe { ec_neg(self.ct as u8, self.dev_ptr(), self.len, result.mem.ptr(), stream()) }, "ec_neg");
        result
    }
}

impl BufferOps for CellBuffer {
    fn from_vec<T: CellEncoding>(data: Vec<T>) -> Self {
        Self::from_host(&data)
    }

    fn with_defaults(len: usize, ct: CellType) -> Self {
        Self::fill(len, ct.zero()) // the `Default` of every cell primitive is its zero
    }

    fn fill(len: usize, value: CellValue) -> Self {
        let filled = Self::uninit(value.cell_type(), len);
        let v = value.to_ffi();
        must(unsafe { ec_fill(filled.ct as u8, filled.mem.ptr(), len, &v, stream()) }, "ec_fill");
        filled
    }

    fn fill_via<T, F>(len: usize, f: F) -> Self
    where
        T: CellEncoding,
        F: Fn(usize) -> T,
    {
        let host: Vec<T> = (0..len).map(f).collect();
        Self::from_host(&host)
    }

    fn len(&self) -> usize {
        self.len
    }

    fn is_empty(&self) -> bool {
        self.len == 0
    }

    fn cell_type(&self) -> CellType {
        self.ct
    }

    fn get(&self, index: usize) -> CellValue {
        self.check_index(index);
        let mut payload = 0u64;
        must(
            unsafe { ec_download(&mut payload as *mut u64 as *mut c_void, self.at(index), self.ct.size_of(), stream()) },
            "ec_download",
        );
        CellValue::from_bits(self.ct, payload)
    }

    fn put(&mut self, idx: usize, value: CellValue) -> Result<()> {
        let payload = value.convert(self.ct)?.bits(); // refused before the bounds check, as in the reference
        self.check_index(idx);
        check(unsafe { ec_upload(self.at(idx), &payload as *const u64 as *const c_void, self.ct.size_of(), stream()) })
    }

    fn convert(&self, cell_type: CellType) -> Result<Self> {
        if cell_type == self.ct {
            return Ok(self.clone());
        }
        if !self.ct.can_fit_into(cell_type) {
            return Err(Error::NarrowingError { src: self.ct, dst: cell_type });
        }
        if self.len == 0 {
            return Ok(Self::empty_u8());
        }
        let widened = Self::uninit(cell_type, self.len);
        check(unsafe { ec_convert(self.ct as u8, self.dev_ptr(), cell_type as u8, widened.mem.ptr(), self.len, stream()) })?;
        Ok(widened)
    }

    fn min_max(&self) -> (CellValue, CellValue) {
        let mut lo = CellValue::UInt8(0).to_ffi();
        let mut hi = lo;
        must(
            unsafe { ec_min_max(self.ct as u8, self.dev_ptr(), std::ptr::null(), self.len, &mut lo, &mut hi, stream()) },
            "ec_min_max",
        );
        (CellValue::from_ffi(&lo), CellValue::from_ffi(&hi))
    }

    fn to_vec<T: CellEncoding>(self) -> Result<Vec<T>> {
        let as_t = self.convert(T::cell_type())?;
        Ok(as_t.fetch::<T>(0, as_t.len)) // `fetch` asserts the cell types agree (an empty convert yields UInt8)
    }
}

impl Clone for CellBuffer {
    fn clone(&self) -> Self {
        self.grown_by(0)
    }
}

impl Debug for CellBuffer {
    /// `UInt8CellBuffer(0, 1, 2, 3, 4, ... 95, 96, 97, 98, 99)`.  More than ten cells: only the first and last five are
    /// downloaded (two small copies), never the buffer.
    fn fmt(&self, f: &mut Formatter<'_>) -> std::fmt::Result {
        write!(f, "{}CellBuffer(", self.ct)?;
        macro_rules! shown {
            ( $(($id:ident, $p:ident)),* ) => {
                match self.ct {
                    $( CellType::$id if self.len > 10 => {
                        let head = self.fetch::<$p>(0, 5);
                        let tail = self.fetch::<$p>(self.len - 5, 5);
                        write!(f, "{:?}, ... {:?}", Elided(&head), Elided(&tail))?
                    }
                    CellType::$id => write!(f, "{:?}", Elided(&self.fetch::<$p>(0, self.len)))?, )*
                }
            };
        }
        with_ct!(shown);
        f.write_str(")")
    }
}

/// `with_ct!` with a third column: the num-traits method that converts a value INTO that primitive.
macro_rules! with_ct_and_to {
    ($callback:ident) => {
        $callback! {
            (UInt8, u8, to_u8), (UInt16, u16, to_u16), (UInt32, u32, to_u32), (UInt64, u64, to_u64),
            (Int8, i8, to_i8), (Int16, i16, to_i16), (Int32, i32, to_i32), (Int64, i64, to_i64),
            (Float32, f32, to_f32), (Float64, f64, to_f64)
        }
    };
}

impl<C: CellEncoding> Extend<C> for CellBuffer {
    /// Items are converted to the buffer's primitive by VALUE (num-traits' range-checked `to_<p>` of [`CellValue`]), not
    /// by cell type: `300u16` does not fit a `UInt8` buffer and panics, `200u16` does.  The whole batch is converted on
    /// the host and appended with one reallocation, one device copy of the old cells and one upload of the new ones.
    fn extend<T: IntoIterator<Item = C>>(&mut self, iter: T) {
        let incoming: Vec<CellValue> = iter.into_iter().map(CellValue::new).collect();
        macro_rules! append {
            ( $(($id:ident, $p:ident, $to:ident)),* ) => {
                match self.ct {
                    $( CellType::$id => {
                        let fitted: Vec<$p> = incoming
                            .iter()
                            .map(|v| v.$to().unwrap_or_else(|| panic!("{v:?} does not fit into a {} cell", self.ct)))
                            .collect();
                        let grown = self.grown_by(fitted.len());
                        upload(grown.at(self.len), &fitted);
                        *self = grown;
                    } )*
                }
            };
        }
        with_ct_and_to!(append);
    }
}

impl<C: CellEncoding> FromIterator<C> for CellBuffer {
    fn from_iter<T: IntoIterator<Item = C>>(iter: T) -> Self {
        let host: Vec<C> = Vec::from_iter(iter);
        Self::from_host(&host)
    }
}

impl FromIterator<CellValue> for CellBuffer {
    /// The FIRST value decides the cell type (no values: `UInt8`); every value must then widen into it — one that does
    /// not panics, as the reference's `get().unwrap()` does.
    fn from_iter<T: IntoIterator<Item = CellValue>>(iterable: T) -> Self {
        let mut values = iterable.into_iter().peekable();
        let Some(decides) = values.peek().map(CellValue::cell_type) else {
            return CellBuffer::with_defaults(0, CellType::UInt8);
        };
        macro_rules! gather {
            ( $(($id:ident, $p:ident)),* ) => {
                match decides {
                    $( CellType::$id => {
                        let host: Vec<$p> = values.map(|v| v.get::<$p>().expect("a value that fits the first value's cell type")).collect();
                        CellBuffer::from_host(&host)
                    } )*
                }
            };
        }
        with_ct!(gather)
    }
}

impl<T: CellEncoding> From<Vec<T>> for CellBuffer {
    fn from(values: Vec<T>) -> Self {
        CellBuffer::from_host(&values)
    }
}

impl<T: CellEncoding> From<&[T]> for CellBuffer {
    fn from(values: &[T]) -> Self {
        CellBuffer::from_host(values)
    }
}

impl<'buf> IntoIterator for &'buf CellBuffer {
    type Item = CellValue;
    type IntoIter = CellBufferIterator<'buf>;

    /// The whole buffer comes over in ONE download; the iterator then decodes cells from that host image.  (Fetching
    /// cell by cell, as an iterator over `get` would, costs a device round trip per cell.)
    fn into_iter(self) -> Self::IntoIter {
        let image = download::<u8>(self.dev_ptr(), self.len * self.ct.size_of());
        CellBufferIterator { of: self, image, next_cell: 0 }
    }
}

/// Walks the cells of a [`CellBuffer`] as [`CellValue`]s over a host image of the buffer.
pub struct CellBufferIterator<'buf> {
    of: &'buf CellBuffer,
    image: Vec<u8>,
    next_cell: usize,
}

impl Iterator for CellBufferIterator<'_> {
    type Item = CellValue;

    fn next(&mut self) -> Option<Self::Item> {
        let width = self.of.ct.size_of();
        let bytes = self.image.get(self.next_cell * width..(self.next_cell + 1) * width)?;
        let mut payload = [0u8; 8];
        payload[..width].copy_from_slice(bytes);
        self.next_cell += 1;
        Some(CellValue::from_bits(self.of.ct, u64::from_le_bytes(payload)))
    }

    fn size_hint(&self) -> (usize, Option<usize>) {
        let left = self.of.len - self.next_cell.min(self.of.len);
        (left, Some(left))
    }
}

impl<C: CellEncoding> TryFrom<CellBuffer> for Vec<C> {
    type Error = Error;

    fn try_from(value: CellBuffer) -> Result<Self> {
        value.to_vec::<C>()
    }
}

/// What [`CellBuffer::composite`] keeps of a cell's stack of layers (`ec_composite_op`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum CompositeOp {
    /// The valid layer with the least index, its bits copied (a priority mosaic).
    First = EC_COMPOSITE_FIRST,
    /// The valid layer with the greatest index.
    Last = EC_COMPOSITE_LAST,
    /// The least valid cell under the total order of `min_max`, its bits copied; equal cells keep the least index.
    Min = EC_COMPOSITE_MIN,
    /// The greatest valid cell.
    Max = EC_COMPOSITE_MAX,
    /// The valid cells added in stack order as `Float64`, one rounded addition each.
    Sum = EC_COMPOSITE_SUM,
    /// The sum divided by the number of valid layers.
    Mean = EC_COMPOSITE_MEAN,
}

impl CompositeOp {
    /// `Float64` for `Sum` and `Mean` (the widening rule of the operators), `cell_type` for the picks.
    pub fn result_type(self, cell_type: CellType) -> CellType {
        match self {
            CompositeOp::Sum | CompositeOp::Mean => CellType::Float64,
            _ => cell_type,
        }
    }
}

impl CellBuffer {
    /// `ec_composite` over `layers` with their mask pointers (`masks` empty: no layer has one; a null entry: that layer has none).
    /// `aux`: also the `UInt8` buffer of where each cell came from.
    pub(crate) fn composite_raw(layers: &[&CellBuffer], masks: &[*const u8], op: CompositeOp, min_count: u32, out_mask: *mut u8, aux: bool) -> Result<(Self, Option<Self>)> {
        assert!(!layers.is_empty() && layers.len() <= EC_COMPOSITE_MAX_LAYERS, "a stack holds 1 .. {EC_COMPOSITE_MAX_LAYERS} layers, not {}", layers.len());
        assert!(masks.is_empty() || masks.len() == layers.len(), "one mask entry per layer");
        let (ct, len) = (layers[0].ct, layers[0].len);
        for l in layers {
            assert_eq!(l.ct, ct, "the layers of a stack share one cell type: cast first");
            assert_eq!(l.len, len, "the layers of a stack share one length");
        }
        let out = Self::uninit(op.result_type(ct), len);
        let source = if aux { Some(Self::uninit(CellType::UInt8, len)) } else { None };
        if len != 0 {
            let cells: Vec<*const c_void> = layers.iter().map(|l| l.dev_ptr()).collect();
            let masks_ptr = if masks.is_empty() { std::ptr::null() } else { masks.as_ptr() };
            let aux_ptr = source.as_ref().map_or(std::ptr::null_mut(), |a| a.mem.ptr() as *mut u8);
            check(unsafe {
                ec_composite(op as i32, ct as u8, cells.as_ptr(), masks_ptr, layers.len() as i32, len, min_count, out.mem.ptr(), out_mask, aux_ptr, stream())
            })?;
        }
        Ok((out, source))
    }

    /// One buffer from a stack of co-registered layers of one cell type and length, in one pass over every layer; the rule is at
    /// `ec_composite` in include/erased_cells.h.  Every cell is valid here: see `MaskedCellBuffer::composite` for clouds.
    pub fn composite(layers: &[&CellBuffer], op: CompositeOp) -> Result<Self> {
        Ok(Self::composite_raw(layers, &[], op, 1, std::ptr::null_mut(), false)?.0)
    }

    /// [`CellBuffer::composite`] and, as `UInt8` cells, the index of the layer each cell came from (for `Sum` / `Mean` the
    /// number of layers counted).
    pub fn composite_with_source(layers: &[&CellBuffer], op: CompositeOp) -> Result<(Self, Self)> {
        let (out, source) = Self::composite_raw(layers, &[], op, 1, std::ptr::null_mut(), true)?;
        Ok((out, source.expect("asked for")))
    }
}

/// How [`CellBuffer::regions`] numbers the regions it keeps (`ec_regions_numbering`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum RegionNumbering {
    /// The region's least row-major cell index plus one.
    Root = EC_REGIONS_ROOT,
    /// 1 .. K in increasing order of that index: `scipy.ndimage.label`'s numbering for a single class.
    Dense = EC_REGIONS_DENSE,
}

/// `ec_regions` over `len` cells read as rows of `cols`, with the workspace from the library's pool: cells (or none: the mask
/// form) and validity bytes (or null) in; the Int32 labels with the number of kept regions (or neither: the sieve-only form) and the
/// validity bytes out.
#[cfg(feature = "masked")]
pub(crate) fn regions_raw(cells: Option<&CellBuffer>, mask: *const u8, len: usize, cols: usize, connectivity: u32, min_cells: u64,
                          numbering: RegionNumbering, labels: bool) -> Result<(Option<(CellBuffer, u64)>, Mask)> {
    assert!(if cols == 0 { len == 0 } else { len % cols == 0 }, "{len} cells are not rows of {cols} cells");
    let out_mask = Mask::uninit(len);
    let out = if labels { Some((CellBuffer::uninit(CellType::Int32, len), CellBuffer::uninit(CellType::UInt64, 1))) } else { None };
    if len == 0 {
        return Ok((out.map(|(l, _)| (l, 0)), out_mask));
    }
    let (t, src) = match cells {
        Some(b) => (b.ct as u8, b.dev_ptr()),
        None => (CellType::UInt8 as u8, std::ptr::null()),
    };
    let (dst, k) = match &out {
        Some((l, k)) => (l.mem.ptr() as *mut i32, k.mem.ptr() as *mut u64),
        None => (std::ptr::null_mut(), std::ptr::null_mut()),
    };
    check(unsafe {
        ec_regions(t, src, mask, cols as u64, (len / cols) as u64, connectivity as i32, numbering as i32, min_cells, dst, out_mask.dev_ptr_mut(), k,
                   std::ptr::null_mut(), stream())
    })?;
    Ok((out.map(|(l, k)| (l, download::<u64>(k.dev_ptr(), 1)[0])), out_mask))
}

#[cfg(feature = "masked")]
impl CellBuffer {
    /// The connected regions of equal cells of this buffer read as rows of `cols` cells (`ec_regions`; the rule is in
    /// include/erased_cells.h): Int32 labels with their validity, and K, the number of regions kept.  "Equal" is equal bits,
    /// `connectivity` is 4 or 8, a region of fewer than `min_cells` cells is invalidated.  The labels are a zone raster:
    /// `zonal_stats(&labels, K + 1)`.
    pub fn regions(&self, cols: usize, connectivity: u32, min_cells: u64, numbering: RegionNumbering) -> Result<(crate::MaskedCellBuffer, u64)> {
        let (out, mask) = regions_raw(Some(self), std::ptr::null(), self.len, cols, connectivity, min_cells, numbering, true)?;
        let (labels, k) = out.expect("asked for");
        Ok((crate::MaskedCellBuffer::new(labels, mask), k))
    }
}

/// Which neighbour [`CellBuffer::composite_rank`] keeps when `q * (count - 1)` is no whole position (`ec_rank_method`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum RankMethod {
    /// The position rounded down: `numpy.quantile`'s "lower".
    Lower = EC_RANK_LOWER,
    /// The position rounded up: "higher".
    Upper = EC_RANK_UPPER,
}

/// The exact fraction `num / den` of [`CellBuffer::composite_rank`]: `(1, 2)` the median, `(0, 1)` the minimum, `(1, 1)` the maximum.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct RankFraction {
    pub num: u32,
    pub den: u32,
}

impl RankFraction {
    pub const MEDIAN: RankFraction = RankFraction { num: 1, den: 2 };
}

impl CellBuffer {
    /// `ec_composite_rank` over `layers` with their mask pointers, as [`CellBuffer::composite_raw`] takes them.
    pub(crate) fn composite_rank_raw(layers: &[&CellBuffer], masks: &[*const u8], q: RankFraction, method: RankMethod, min_count: u32, out_mask: *mut u8,
                                     aux: bool) -> Result<(Self, Option<Self>)> {
        assert!(!layers.is_empty() && layers.len() <= EC_COMPOSITE_MAX_LAYERS, "a stack holds 1 .. {EC_COMPOSITE_MAX_LAYERS} layers, not {}", layers.len());
        assert!(masks.is_empty() || masks.len() == layers.len(), "one mask entry per layer");
        assert!(q.den >= 1 && q.den <= EC_RANK_MAX_DEN && q.num <= q.den, "q = {} / {} needs 1 <= den <= {EC_RANK_MAX_DEN} and num <= den", q.num, q.den);
        let (ct, len) = (layers[0].ct, layers[0].len);
        for l in layers {
            assert_eq!(l.ct, ct, "the layers of a stack share one cell type: cast first");
            assert_eq!(l.len, len, "the layers of a stack share one length");
        }
        let out = Self::uninit(ct, len);
        let source = if aux { Some(Self::uninit(CellType::UInt8, len)) } else { None };
        if len != 0 {
            let cells: Vec<*const c_void> = layers.iter().map(|l| l.dev_ptr()).collect();
            let masks_ptr = if masks.is_empty() { std::ptr::null() } else { masks.as_ptr() };
            let aux_ptr = source.as_ref().map_or(std::ptr::null_mut(), |a| a.mem.ptr() as *mut u8);
            check(unsafe {
                ec_composite_rank(ct as u8, cells.as_ptr(), masks_ptr, layers.len() as i32, len, q.num, q.den, method as i32, min_count, out.mem.ptr(),
                                  out_mask, aux_ptr, stream())
            })?;
        }
        Ok((out, source))
    }

    /// The per-cell order statistic of a stack of co-registered layers of one cell type and length, in one pass: the cells of each
    /// stack in the total order of `min_max`, ties by layer index, and the one at position `q * (layers - 1)` kept; the rule is at
    /// `ec_composite_rank` in include/erased_cells.h.  Every cell is valid here: see `MaskedCellBuffer::composite_rank` for clouds.
    pub fn composite_rank(layers: &[&CellBuffer], q: RankFraction, method: RankMethod) -> Result<Self> {
        Ok(Self::composite_rank_raw(layers, &[], q, method, 1, std::ptr::null_mut(), false)?.0)
    }

    /// [`CellBuffer::composite_rank`] at one half: the lower or the upper median.
    pub fn composite_median(layers: &[&CellBuffer], method: RankMethod) -> Result<Self> {
        Self::composite_rank(layers, RankFraction::MEDIAN, method)
    }

    /// [`CellBuffer::composite_rank`] and, as `UInt8` cells, the index of the layer each cell came from.
    pub fn composite_rank_with_source(layers: &[&CellBuffer], q: RankFraction, method: RankMethod) -> Result<(Self, Self)> {
        let (out, source) = Self::composite_rank_raw(layers, &[], q, method, 1, std::ptr::null_mut(), true)?;
        Ok((out, source.expect("asked for")))
    }
}

// api-surface(src/buffer.rs:318-436): the sixteen binary-operator impl headers, the two `Neg` impls and the ordering /
// equality impl headers of CellBuffer (`&a op &b`, `a op b`, `a op &b`, `a op scalar`; no `scalar op a` in the reference either)
macro_rules! buffer_operator {
    ($trt:ident, $mth:ident, $code:expr) => {
        impl $trt for &CellBuffer {
            type Output = CellBuffer;
            fn $mth(self, rhs: Self) -> Self::Output {
                self.binop($code, rhs)
            }
        }
        impl $trt for CellBuffer {
            type Output = CellBuffer;
            fn $mth(self, rhs: Self) -> Self::Output {
                self.binop($code, &rhs)
            }
        }
        impl $trt<&CellBuffer> for CellBuffer {
            type Output = CellBuffer;
            fn $mth(self, rhs: &CellBuffer) -> Self::Output {
                self.binop($code, rhs)
            }
        }
        impl<R> $trt<R> for CellBuffer
        where
            R: Into<CellValue>,
        {
            type Output = CellBuffer;
            fn $mth(self, rhs: R) -> Self::Output {
                self.binop_scalar($code, rhs.into())
            }
        }
    };
}
buffer_operator!(Add, add, EC_ADD);
buffer_operator!(Sub, sub, EC_SUB);
buffer_operator!(Mul, mul, EC_MUL);
buffer_operator!(Div, div, EC_DIV);

impl Neg for &CellBuffer {
    type Output = CellBuffer;
    fn neg(self) -> Self::Output {
        self.negated()
    }
}

impl Neg for CellBuffer {
    type Output = CellBuffer;
    fn neg(self) -> Self::Output {
        self.negated()
    }
}

impl PartialEq<Self> for CellBuffer {
    fn eq(&self, other: &Self) -> bool {
        self.cmp(other).is_eq()
    }
}

impl Eq for CellBuffer {}

impl PartialOrd for CellBuffer {
    fn partial_cmp(&self, other: &Self) -> Option<Ordering> {
        Some(Ord::cmp(self, other))
    }
}

impl Ord for CellBuffer {
    /// Cell type first; then the first pair of differing cells decides, under the total order (`total_cmp` for floats,
    /// so equality is bit equality); then length.  Decided on the device (`ec_buffer_cmp`: a first-difference
    /// reduction) — no cell is downloaded.
    fn cmp(&self, other: &Self) -> Ordering {
        let mut sign = 0i32;
        must(
            unsafe { ec_buffer_cmp(self.ct as u8, self.dev_ptr(), self.len, other.ct as u8, other.dev_ptr(), other.len, &mut sign, stream()) },
            "ec_buffer_cmp",
        );
        sign.cmp(&0)
    }
}
// end api-surface

impl CellBuffer {
    /// `ec_zonal_stats_compute`: [`CellBuffer::stats`] per zone of the zone raster `zones` (`UInt8`, `UInt16` or `Int32`, one id per
    /// cell) in one pass.  `mask`: the device bytes of a mask of the same length, or null.
    pub(crate) fn zonal_stats_raw(&self, mask: *const u8, zones: &CellBuffer, n_zones: usize) -> Result<Vec<Stats>> {
        assert_eq!(zones.len, self.len, "the zone raster and the values share one length");
        assert!((1..=EC_ZONAL_MAX_ZONES).contains(&n_zones), "1 .. {EC_ZONAL_MAX_ZONES} zones, not {n_zones}: relabel in chunks");
        let mut out = vec![Stats::blank(); n_zones];
        check(unsafe {
            ec_zonal_stats_compute(self.ct as u8, self.dev_ptr(), mask, zones.ct as u8, zones.dev_ptr(), self.len, n_zones as i32,
                                   out.as_mut_ptr() as *mut c_void, stream())
        })?;
        Ok(out.iter().map(Stats::from_ffi).collect())
    }

    /// Entry `z` holds the statistics of the cells whose id in `zones` is `z`; an id outside `0 .. n_zones` belongs to no zone.
    /// The rule is at `ec_zonal_stats_device` in include/erased_cells.h.
    pub fn zonal_stats(&self, zones: &CellBuffer, n_zones: usize) -> Result<Vec<Stats>> {
        self.zonal_stats_raw(std::ptr::null(), zones, n_zones)
    }

    /// This buffer as a zone raster, each cell replaced by `table[id]` (`ec_zonal_broadcast`): the cells and the mask of where an
    /// id was inside `0 .. table.len()`; every other cell is zero and not valid.  `MaskedCellBuffer::broadcast` pairs them.
    pub fn broadcast(&self, table: &CellBuffer) -> Result<(CellBuffer, Mask)> {
        assert!((1..=EC_ZONAL_MAX_ZONES).contains(&table.len), "a table of 1 .. {EC_ZONAL_MAX_ZONES} cells, not {}", table.len);
        let out = Self::uninit(table.ct, self.len);
        let mask = Mask::uninit(self.len);
        check(unsafe {
            ec_zonal_broadcast(self.ct as u8, self.dev_ptr(), self.len, table.len as i32, table.ct as u8, table.dev_ptr(), out.mem.ptr(),
                               mask.dev_ptr_mut(), stream())
        })?;
        Ok((out, mask))
    }

    /// `ec_zonal_table_compute`: [`CellBuffer::zonal_stats`] for up to `EC_ZONAL_TABLE_MAX_ZONES` zones, over a per-zone table in
    /// device memory.  `mask`: the device bytes of a mask of the same length, or null.
    pub(crate) fn zonal_table_raw(&self, mask: *const u8, zones: &CellBuffer, n_zones: usize) -> Result<Vec<Stats>> {
        assert_eq!(zones.len, self.len, "the zone raster and the values share one length");
        assert!((1..=EC_ZONAL_TABLE_MAX_ZONES).contains(&n_zones), "1 .. {EC_ZONAL_TABLE_MAX_ZONES} zones, not {n_zones}");
        let mut out = vec![Stats::blank(); n_zones];
        check(unsafe {
            ec_zonal_table_compute(self.ct as u8, self.dev_ptr(), mask, zones.ct as u8, zones.dev_ptr(), self.len, n_zones as i32,
                                   out.as_mut_ptr() as *mut c_void, stream())
        })?;
        Ok(out.iter().map(Stats::from_ffi).collect())
    }

    /// [`CellBuffer::zonal_stats`] for up to `EC_ZONAL_TABLE_MAX_ZONES` zones — the labels of [`CellBuffer::regions`], a `UInt16` parcel
    /// raster.  The rule, whose float and 64-bit sums are truncated fixed-point sums independent of any order, is at
    /// `ec_zonal_table_device` in include/erased_cells.h.
    pub fn zonal_table(&self, zones: &CellBuffer, n_zones: usize) -> Result<Vec<Stats>> {
        self.zonal_table_raw(std::ptr::null(), zones, n_zones)
    }

    /// [`CellBuffer::broadcast`] for a table of up to `EC_ZONAL_TABLE_MAX_ZONES` cells, read from device memory (`ec_zonal_lookup`).
    pub fn lookup(&self, table: &CellBuffer) -> Result<(CellBuffer, Mask)> {
        assert!((1..=EC_ZONAL_TABLE_MAX_ZONES).contains(&table.len), "a table of 1 .. {EC_ZONAL_TABLE_MAX_ZONES} cells, not {}", table.len);
        let out = Self::uninit(table.ct, self.len);
        let mask = Mask::uninit(self.len);
        check(unsafe {
            ec_zonal_lookup(self.ct as u8, self.dev_ptr(), self.len, table.len as i32, table.ct as u8, table.dev_ptr(), out.mem.ptr(),
                            mask.dev_ptr_mut(), stream())
        })?;
        Ok((out, mask))
    }
}

/// The table of [`CellBuffer::reclassify`] for rasters of one cell type: built on the host (`ec_reclass_table_build`), uploaded once,
/// reusable across calls on this device.  The rule is at `ec_reclass` in include/erased_cells.h.
pub struct ReclassTable {
    pub(crate) host: Box<ec_reclass_table>,
    pub(crate) mem: DeviceMem,
}

impl ReclassTable {
    /// `breaks`: 1 ..= 255 cells of type `B`, strictly ascending in the union with `cell_type`, none NaN; `values`: one cell of the
    /// output type `D` per class (`breaks.len() + 1`); `valid`: empty, or one flag per class — a false one drops its class;
    /// `nodata`: given iff the table is for [`MaskedCellBuffer`]s, what a cell that is not valid receives.
    pub fn new<B: CellEncoding, D: CellEncoding>(
        cell_type: CellType, breaks: &[B], values: &[D], right: bool, valid: &[bool], nodata: Option<D>,
    ) -> Result<Self> {
        assert!((1..=EC_RECLASS_MAX_BREAKS).contains(&breaks.len()), "1 .. {EC_RECLASS_MAX_BREAKS} breaks, not {}", breaks.len());
        assert_eq!(values.len(), breaks.len() + 1, "one class value more than there are breaks");
        assert!(valid.is_empty() || valid.len() == values.len(), "one validity flag per class");
        let vals: Vec<ec_value> = values.iter().map(|v| CellValue::new(*v).to_ffi()).collect();
        let flags: Vec<u8> = valid.iter().map(|v| *v as u8).collect();
        let marker = nodata.map(|v| CellValue::new(v).to_ffi());
        let mut host: Box<ec_reclass_table> = Box::new(unsafe { std::mem::zeroed() });
        check(unsafe {
            ec_reclass_table_build(cell_type as u8, B::cell_type() as u8, breaks.as_ptr() as *const c_void, breaks.len() as i32, right as i32,
                                   D::cell_type() as u8, vals.as_ptr(), if flags.is_empty() { std::ptr::null() } else { flags.as_ptr() },
                                   marker.as_ref().map_or(std::ptr::null(), |m| m as *const ec_value),
                                   &mut *host as *mut ec_reclass_table as *mut c_void)
        })?;
        let mem = DeviceMem::new(EC_RECLASS_TABLE_BYTES);
        upload(mem.ptr(), std::slice::from_ref(&*host));
        Ok(ReclassTable { host, mem })
    }

    pub fn cell_type(&self) -> CellType {
        CellType::from_code(self.host.t as u8)
    }
    pub fn result_type(&self) -> CellType {
        CellType::from_code(self.host.dt as u8)
    }
    pub fn has_nodata(&self) -> bool {
        self.host.flags & EC_RECLASS_HAS_NODATA != 0
    }
    pub fn drops(&self) -> bool {
        self.host.flags & EC_RECLASS_DROPS != 0
    }
}

impl CellBuffer {
    /// `ec_reclass` of these cells under `mask` (device bytes, or null) into a new buffer, with the result's mask when asked for.
    pub(crate) fn reclass_raw(&self, mask: *const u8, table: &ReclassTable, want_mask: bool) -> Result<(CellBuffer, Option<Mask>)> {
        assert_eq!(table.cell_type(), self.ct, "the table is for rasters of another cell type");
        assert_eq!(table.has_nodata(), !mask.is_null(), "a table built with a nodata value is for masked rasters, one without for plain ones");
        assert!(want_mask || !table.drops(), "a table that drops a class needs the result's mask");
        let out = Self::uninit(table.result_type(), self.len);
        let om = if want_mask { Some(Mask::uninit(self.len)) } else { None };
        check(unsafe {
            ec_reclass(self.ct as u8, self.dev_ptr(), mask, self.len, table.result_type() as u8, table.mem.ptr(), out.mem.ptr(),
                       om.as_ref().map_or(std::ptr::null_mut(), |m| m.dev_ptr_mut()), stream())
        })?;
        Ok((out, om))
    }

    /// Each cell replaced by the value of its class among the table's breaks, in one pass.  The table drops no class (that form
    /// is [`MaskedCellBuffer::reclassify`]'s).
    pub fn reclassify(&self, table: &ReclassTable) -> Result<CellBuffer> {
        Ok(self.reclass_raw(std::ptr::null(), table, false)?.0)
    }

    /// A `UInt8` class raster with values `0 ..= breaks.len()`: class `c` = the number of breaks `<=` the cell (`right`: `<`) under
    /// the reference's total order — fit for [`CellBuffer::zonal_stats`], whose counts are then a histogram.
    pub fn classify<B: CellEncoding>(&self, breaks: &[B], right: bool) -> Result<CellBuffer> {
        let ids: Vec<u8> = (0..=breaks.len()).map(|c| c as u8).collect();
        self.reclassify(&ReclassTable::new::<B, u8>(self.ct, breaks, &ids, right, &[], None)?)
    }
}
