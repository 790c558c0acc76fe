/*
 * hipims_mi.h -- C ABI of the MI355X-native shallow-water step engine (libhipims_mi.so).
 *
 * This is the drop-in boundary for ONE path of HiPIMS-OCL (lukeshope/hipims-ocl): the per-timestep
 * update that `CSchemeGodunov` / `CSchemeMUSCLHancock` / `CSchemeInertial` drive through the OpenCL executor classes
 * (`COCLProgram`, `COCLKernel`, `COCLBuffer`, `COCLDevice`).  The HIP engine owns the kernel graph,
 * so the reference's generic program/kernel/argument layer collapses into semantic calls; each
 * entry point below cites the reference interface it replaces (paths relative to the reference's
 * `src/`).  INTEGRATION.md shows the binding a HiPIMS maintainer would add.
 *
 * Conventions
 *  - plain C, plain pointers and sizes; no C++/torch types cross this boundary;
 *  - every function returns 0 (HP_OK) or a negative hp_status; hp_last_error() gives the message of
 *    the calling thread's last failure.  Nothing throws, nothing calls exit() (the reference's
 *    model::doError levels, main.cpp:631-652, are left to the host);
 *  - host arrays use the reference's layout unchanged (Domain/CDomain.h:26-33, CDomain.cpp:171-180):
 *    state = cols*rows x {Z free-surface level, Zmax, Qx, Qy}, row-major, row 0 = south;
 *    bed / manning = cols*rows scalars.  Element type = double (precision 8) or float (precision 4);
 *  - transfers and steps are ASYNCHRONOUS on the domain's HIP stream, exactly like the reference's
 *    non-blocking queueWrite / queueRead / scheduleExecution: host memory passed to upload/download
 *    must stay alive until hp_sync() (COCLDevice::blockUntilFinished) returns;
 *  - threading contract = the reference's (Schemes/CSchemeGodunov.cpp:1116-1370): one worker thread
 *    per domain may call step/read/sync; hp_is_busy may be called from another thread; everything
 *    else requires the domain to be idle.
 *  - there is NO CPU fallback: every call fails with HP_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef HIPIMS_MI_H
#define HIPIMS_MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HP_ABI_VERSION 2          /* 2: hp_domain_desc_t.ghost_rows */

typedef enum {
	HP_OK              =  0,
	HP_ERR_INVALID     = -1,    /* bad argument / descriptor */
	HP_ERR_NO_DEVICE   = -2,    /* no usable HIP device (never falls back to the CPU) */
	HP_ERR_HIP         = -3,    /* a HIP runtime call failed; see hp_last_error() */
	HP_ERR_UNSUPPORTED = -4,
	HP_ERR_STATE       = -5     /* call not valid in the domain's current state */
} hp_status;

/* Schemes: Schemes/CScheme.cpp:141-190 (createFromConfig "Godunov" / "MUSCL-Hancock") */
enum { HP_SCHEME_GODUNOV = 0, HP_SCHEME_MUSCL_HANCOCK = 1, HP_SCHEME_INERTIAL = 2 };   /* model::schemeTypes, CScheme.h:33-37 */

/* which array an upload / download moves: COCLBuffer "Cell states", "Bed elevations",
 * "Manning coefficients" (Schemes/CSchemeGodunov.cpp:832-845) */
enum { HP_ARRAY_STATE = 0, HP_ARRAY_BED = 1, HP_ARRAY_MANNING = 2 };

/* Behaviours of the reference a parity run reproduces; each can be switched off.
 * HP_QUIRKS_REFERENCE is the default and is what the parity tests run. */
enum {
	HP_QUIRK_CFL_READS_PRIMARY = 1u << 0,  /* Q1: tst_Reduce always reads the primary state buffer
	                                          (CSchemeGodunov.cpp:1629/:1634 set a non-existent arg) */
	HP_QUIRK_BDY_TRUNCATED     = 1u << 1,  /* Q9: boundary kernels cover floor(n/8)*8 cells per axis
	                                          (Boundaries/CBoundaryUniform.cpp:294-295) */
	HP_QUIRK_MUSCL_NEIGHBOUR_Y_IS_BED = 1u << 2,
	                                       /* Q11: the reference's DEFAULT MUSCL-Hancock configuration is kCachePrediction
	                                          (Schemes/CSchemeMUSCLHancock.cpp:46): mch_1st_cachePrediction keeps {Z, BED, Qx, Qy}
	                                          in LDS (CLSchemeMUSCLHancock.clc:201) and hands the four neighbours to mch_1st with
	                                          their bed in .y (:232-239), so the predictor's first-order fallback
	                                          `pNeigData*.y <= -9998.0` (:325-330) tests the neighbour's BED -- a cell next to a
	                                          disabled (Zmax = -9999) cell with an ordinary bed stays second order.  Off = the
	                                          non-default mch_1st_cacheNone variant, which tests the neighbour's Zmax (:109-125). */
	HP_QUIRKS_REFERENCE        = 7u
};

/* Arithmetic flavour of the device kernels.
 *  STRICT: the reference's expression order, IEEE division/sqrt, no FMA contraction -- bit-identical to
 *          the oracle and to the reference's own kernels as built by oracle/ref_build, friction included: pow(), the one
 *          built-in whose result is implementation defined, is in all three the correctly rounded cube root of
 *          csrc/hp_crmath.h (i.e. the identity holds against the reference run on a platform with THAT pow; a
 *          platform with another conforming pow differs in the last bit of the friction term, fixture f10_*_libm);
 *  FAST  : algebraically identical, fewer divisions, explicit FMAs (the reference itself ships with
 *          -cl-mad-enable, OpenCL/Executors/COCLProgram.cpp:73, so its own results are compiler
 *          dependent at this level).  Default. */
enum { HP_MATH_FAST = 0, HP_MATH_STRICT = 1 };

/* Kernel selection (diagnostics): AUTO = the tuned kernel; BASIC = one thread per cell, four face
 * solves per cell -- the same dataflow as gts_cacheDisabled, kept as an on-device cross-check. */
enum { HP_KERNEL_AUTO = 0, HP_KERNEL_BASIC = 1 };

typedef struct hp_domain hp_domain_t;

/* ---- device discovery: COCLDevice capability fields (OpenCL/Executors/COCLDevice.h:53-99),
 *      CExecutorControlOpenCL::createDevices (CExecutorControlOpenCL.cpp:211) ---- */
typedef struct {
	char     name[128];          /* clDeviceName */
	char     arch[32];           /* gcnArchName, e.g. "gfx950" */
	int32_t  compute_units;      /* clDeviceComputeUnits */
	int32_t  clock_mhz;          /* clDeviceClockFrequency */
	uint64_t global_mem_bytes;   /* clDeviceGlobalMemSize */
	uint64_t lds_bytes_per_cu;   /* clDeviceLocalSize */
	int32_t  wavefront;          /* 64 on gfx950 */
	int32_t  fp64;               /* COCLDevice::isDoubleCompatible */
} hp_device_info_t;

int hp_abi_version(void);
int hp_device_count(int* count);
int hp_device_info(int device, hp_device_info_t* info);
const char* hp_last_error(void);

/* Optional log sink, the place model::doError (src/main.cpp:631-652 -> CLog::writeError) has in the reference: every
 * failing call hands its message to `sink` with the reference's error level (common.h:62-68; failures of this
 * library are kLevelModelStop = 2) before returning its code, so an adapter can forward to pManager->log without
 * polling hp_last_error().  Process-wide; NULL removes it.  Called on the thread that made the failing call. */
#define HP_LOG_FATAL        1
#define HP_LOG_MODEL_STOP   2
#define HP_LOG_CONTINUE     4
#define HP_LOG_WARNING      8
#define HP_LOG_INFORMATION 16
typedef void (*hp_log_sink_t)(int level, const char* message, void* user);
int hp_set_log_sink(hp_log_sink_t sink, void* user);

/* ---- domain: CScheme::prepareAll + the registerConstant set
 *      (Schemes/CSchemeGodunov.cpp:386-470, :666-784; XML parameters :128-333, CScheme.cpp:46-55) ---- */
typedef struct {
	uint32_t struct_size;        /* = sizeof(hp_domain_desc_t) */
	int32_t  device;             /* <domain deviceNumber=...> (Domain/CDomainManager.cpp:203-220) */
	int64_t  cols, rows;         /* LOCAL array size (all rows this rank stores, ghosts included) */
	double   dx;                 /* cell resolution; DOMAIN_DELTAX == DOMAIN_DELTAY */
	int32_t  precision;          /* 8 (fp64) or 4 (fp32): <simulation floatingPointPrecision> */
	int32_t  scheme;             /* HP_SCHEME_* */
	double   courant;            /* courantNumber, default 0.5 */
	double   dry_threshold;      /* dryThreshold = VERY_SMALL, default 1e-10; QUITE_SMALL = 10x */
	int32_t  friction;           /* frictionEffects (fused into the flux kernel) */
	int32_t  dynamic_dt;         /* timestepMode: 1 = CFL, 0 = fixed */
	double   dt_fixed;           /* TIMESTEP_FIXED */
	double   dt_initial;         /* timestepInitial, default 0.001 */
	double   t_end;              /* simulation duration = SCHEME_ENDTIME */
	uint32_t quirks;             /* HP_QUIRK_* mask */
	int32_t  math_mode;          /* HP_MATH_* */
	int32_t  kernel;             /* HP_KERNEL_* */
	/* 1-D row-strip decomposition (replaces Domain/Links/CDomainLink + MPI).
	 * A single-GPU domain has global_rows == rows and row_offset == 0. */
	int64_t  global_rows;        /* rows of the whole logical grid */
	int64_t  row_offset;         /* global row index of local row 0 */
	/* Ghost rows stored per interior side of a strip: 0 = one stencil reach g (1 row Godunov / inertial, 2 MUSCL-Hancock) and a
	 * ghost-row exchange after every iteration; 2g = two reaches and an exchange after every SECOND iteration (the strip
	 * recomputes g of its neighbour's rows redundantly in between; hp_strip_step_batch only).  What is left of the reference's
	 * wide overlap zones with several iterations between synchronisations (Domain/Links/CDomainLink.cpp:297-328,
	 * Domain/CDomainBase.cpp:163-174), here without forecast and rollback: results stay bit-identical to the single domain. */
	int32_t  ghost_rows;
	int32_t  reserved0;
} hp_domain_desc_t;

void hp_domain_desc_default(hp_domain_desc_t* desc);   /* reference defaults, CScheme.cpp:46-55 */
int  hp_domain_create(const hp_domain_desc_t* desc, hp_domain_t** out);
int  hp_domain_destroy(hp_domain_t* d);                /* CSchemeGodunov::release1OResources, :993-1048 */

/* COCLBuffer::queueWriteAll (COCLBuffer.h:40): HP_ARRAY_STATE fills BOTH ping-pong buffers, as
 * prepareSimulation does (CSchemeGodunov.cpp:1064-1065), and resets the ping-pong phase. */
int hp_domain_upload(hp_domain_t* d, int which, const void* host, size_t bytes);
/* COCLBuffer::queueReadAll / queueReadPartial (COCLBuffer.h:38-43); for HP_ARRAY_STATE reads the buffer
 * the NEXT iteration would use as its source (CSchemeGodunov::getNextCellSourceBuffer, :1705-1715,
 * which is what readDomainAll / saveCurrentState / CDomainLink::pullFromBuffer read). */
int hp_domain_download(hp_domain_t* d, int which, void* host, int64_t row0, int64_t nrows);
/* COCLBuffer::queueWritePartial into the next source buffer (CDomainLink::pushToBuffer, CDomainLink.cpp:252-270) */
int hp_domain_upload_rows(hp_domain_t* d, const void* host, int64_t row0, int64_t nrows);

/* ---- the output stage on the device (no state download).
 *      CDomainCartesian::writeOutputs (Domain/Cartesian/CDomainCartesian.cpp:804-829) reads the whole cell state back and
 *      derives every raster on the host (Datasets/CRasterDataset.cpp:185-267); hp_domain_derive derives them where the
 *      state lives and moves only the rasters asked for (8 or 4 bytes per cell and raster instead of 32 / 16 per cell).
 *      All arithmetic is fp64 whatever the domain's precision (an fp32 domain's values are widened first) and uses
 *      correctly rounded operations only: the fp64 rasters equal the host derivation bit for bit, the fp32 ones are
 *      those values rounded once.  NODATA = -9999, wet threshold 1e-8 (the reference's, not dryThreshold). ---- */
enum { HP_OUT_DEPTH = 0, HP_OUT_MAXDEPTH = 1, HP_OUT_FSL = 2, HP_OUT_MAXFSL = 3, HP_OUT_DISCHARGE_X = 4, HP_OUT_DISCHARGE_Y = 5,
       HP_OUT_VELOCITY_X = 6, HP_OUT_VELOCITY_Y = 7, HP_OUT_FROUDE = 8, HP_OUT_COUNT = 9 };
/* rasters[i] receives value values[i] (each value at most once) for rows [row0, row0 + nrows) of the LOCAL array (a strip's
 * ghost rows included: the caller picks the owned range), cols elements a row, row 0 = south, element_bytes 8 (double) or
 * 4 (float).  Reads the buffer hp_domain_download(HP_ARRAY_STATE) reads, in stream order behind whatever is queued, and
 * changes nothing the steps depend on.  Enqueued on the domain's stream like hp_domain_download: the host memory must
 * stay alive until hp_sync().  Device scratch for the rasters is allocated on first use and bounded (256 MiB: larger
 * requests are worked through in blocks of rows); if that allocation fails the call returns HP_ERR_HIP and the domain
 * stays usable.  Argument errors are HP_ERR_INVALID before any device call; nrows == 0 is HP_OK. */
int hp_domain_derive(hp_domain_t* d, const int* values, int count, int element_bytes,
                     void* const* rasters, int64_t row0, int64_t nrows);
/* The same nine values aggregated over square blocks of factor x factor cells on the device: an overview of the run (a progress
 * map, the frames of an animation) for 1 / factor^2 of the bytes a full raster moves to the host.  No reference counterpart.
 *   Blocks.  Block (bx, by) holds the cells with x / factor == bx and (row_offset + y) / factor == by: blocks are anchored to the
 * GLOBAL grid, so that the overviews of strips can be put together.  factor is any integer in 1..4096 -- no power of two, no
 * divisor of the grid; it may exceed cols or rows.  block_cols = ceil(cols / factor), first_block_row = (row_offset + row0) /
 * factor, block_rows = the block rows touched by rows [row0, row0 + nrows) of the LOCAL array (0 for nrows == 0):
 * hp_overview_shape, pure arithmetic without a device call.  rasters[i] receives block_rows * block_cols elements, row 0 = south.
 * Only cells inside the row range take part (a strip's caller picks the owned range): edge blocks are partial.
 *   Per-cell value.  That of values[i] (HP_OUT_*) is exactly what hp_domain_derive forms in fp64 before it rounds: the same
 * expressions, NODATA rules and 1e-8 wet test (one definition in csrc/hp_output.hpp serves both).
 *   Aggregation.  A cell takes part in a block iff its value is neither -9999.0 nor a NaN.  HP_AGG_MAX / HP_AGG_MIN: the largest /
 * smallest participating value (values are signed; -0.0 lies below +0.0), -9999.0 if there is none.  HP_AGG_COUNT: the number of
 * participating cells, as an exactly representable floating-point number.  element_bytes 8 delivers these fp64 results, 4 the same
 * results rounded once, after the aggregation.  All three are order-independent -- what is accumulated is integers: an
 * order-preserving key of the double, and counts; there is no floating-point atomic and no floating-point sum -- so the result
 * depends neither on the launch shape nor on how a large request is cut into runs of block rows nor on how the grid is cut into
 * strips (frontend.overview restates it in NumPy, frontend.combine_overviews puts the parts of strips or row ranges together).
 *   Each (value, aggregate) pair at most once; count is 1..27.  Everything else follows hp_domain_derive: reads the buffer
 * hp_domain_download(HP_ARRAY_STATE) reads, in stream order behind whatever is queued, changes nothing the steps depend on, is
 * enqueued on the domain's stream and never blocks; the host memory must stay alive until hp_sync().  The accumulators and the
 * elements come out of the same bounded scratch (256 MiB; larger requests are worked through in runs of whole block rows).
 * Argument errors -- a NULL pointer, an unknown value or aggregate, a repeated pair, a factor outside 1..4096, a bad
 * element_bytes, a row range outside the array -- are HP_ERR_INVALID before any device call; between hp_step_begin and
 * hp_step_end the call returns HP_ERR_STATE; nrows == 0 is HP_OK. */
enum { HP_AGG_MAX = 0, HP_AGG_MIN = 1, HP_AGG_COUNT = 2, HP_AGG_KINDS = 3 };
int hp_overview_shape(hp_domain_t* d, int factor, int64_t row0, int64_t nrows,
                      int64_t* first_block_row, int64_t* block_rows, int64_t* block_cols);
int hp_domain_overview(hp_domain_t* d, const int* values, const int* aggregates, int count,
                       int factor, int element_bytes, void* const* rasters,
                       int64_t row0, int64_t nrows);
/* The same nine values at the SELECTED cells only, at full resolution, in CSR: a flood map is mostly -9999, and what a user
 * takes away from an output time is depth and velocity where there is water.  Only the selected share of a raster's bytes crosses
 * the host link.  No reference counterpart.
 *   Selection.  Cell (x, y) of rows [row0, row0 + nrows) of the LOCAL array is selected iff v, the value select_value (HP_OUT_*)
 * of that cell exactly as hp_domain_derive forms it in fp64 before it rounds (one definition in csrc/hp_output.hpp serves both),
 * satisfies v != -9999.0 && v > above.  A NaN v fails the comparison.  above may be -inf (HP_OUT_DISCHARGE_X, -inf selects every
 * cell: that value is never NODATA); typical use is HP_OUT_DEPTH, 0.01.
 *   Result.  row_ptr[0 .. nrows]: row_ptr[0] = 0 and row_ptr[r + 1] - row_ptr[r] = the selected cells of local row row0 + r;
 * *selected = row_ptr[nrows].  col[k] is the column of entry k; entries ascend by (row, column).  rasters[i][k] is value values[i]
 * of entry k: element_bytes 8 delivers the fp64 value, 4 the same value rounded once -- the elements hp_domain_derive stores.  A
 * selected cell's other values may themselves be -9999 (maxdepth at a wall): they are delivered as they are.  Each value at most
 * once; count is 1..9.
 *   Capacity.  row_ptr and *selected are always delivered.  If *selected > capacity, nothing is written to col or rasters and the
 * call still returns HP_OK: the caller grows its arrays and calls again.  capacity == 0 with col and rasters NULL is the counting
 * call.
 *   The call BLOCKS, like hp_domain_stats: behind the scan the host reads row_ptr, and only then are the copies queued, of exactly
 * *selected entries each.  On return row_ptr and *selected are valid; col and rasters are valid after hp_sync() -- their copies
 * are enqueued on the domain's stream and the host memory must stay alive until then, as for hp_domain_derive.
 *   Everything else follows hp_domain_overview: reads the buffer hp_domain_download(HP_ARRAY_STATE) reads, in stream order behind
 * whatever is queued, and changes nothing the steps depend on.  What is accumulated is integers (a ballot per 64 columns, its
 * population counts, their prefix sums), so the result depends neither on the launch shape nor on how a large request is cut into
 * runs nor on how the grid is cut into strips (frontend.sparse restates it in NumPy, frontend.combine_sparse concatenates the parts
 * of consecutive row ranges).  The selection words and offsets (16 B per 64 cells) and the entries (4 + count * element_bytes B
 * each) come out of the same bounded scratch (256 MiB): a range whose words alone exceed it is HP_ERR_UNSUPPORTED, entries that
 * exceed what is left are worked through in runs of whole rows (a row larger than that in runs of entries).  If an allocation
 * fails the call returns HP_ERR_HIP and the domain stays usable.  Argument errors -- a NULL selected or row_ptr; capacity > 0 with
 * a NULL col, rasters or rasters[i]; an unknown or repeated value; an unknown select_value; a bad element_bytes; a NaN above; a
 * row range outside the array; cols >= 2^32 -- are HP_ERR_INVALID before any device call; between hp_step_begin and hp_step_end
 * the call returns HP_ERR_STATE; nrows == 0 is HP_OK with *selected = 0 and row_ptr[0] = 0. */
int hp_domain_sparse(hp_domain_t* d, int select_value, double above,
                     const int* values, int count, int element_bytes,
                     uint64_t capacity, uint64_t* selected,
                     uint64_t* row_ptr, uint32_t* col, void* const* rasters,
                     int64_t row0, int64_t nrows);
/* Statistics of rows [row0, row0 + nrows) of the same buffer: what the reference's progress log takes from
 * CDomainCartesian::getVolume (CDomainCartesian.cpp:743-760, CSchemeGodunov.cpp:1060, CModel.cpp:1127) and what a user
 * reads next to it.  A deterministic two-stage reduction (no floating-point atomics: the same state gives the same bits). */
typedef struct {
	uint32_t struct_size;        /* = sizeof(hp_domain_stats_t), set by the caller */
	uint32_t reserved;
	uint64_t cells;              /* cells counted: not disabled (Zmax > -9999) and bed <= 9999 (closed-edge walls hold no water) */
	uint64_t cells_wet;          /* counted cells with Z - bed > 1e-8 */
	double   volume;             /* dx^2 * sum of max(0, Z - bed) over the counted cells, m3.  NOT getVolume's sum, which is
	                                unclamped (cells whose level lies below their bed count negative) and includes the walls
	                                and disabled cells */
	double   max_depth;          /* largest max(0, Z - bed) of a counted cell (0 if none is counted) */
	double   max_speed;          /* largest sqrt(vx^2 + vy^2), v = Q / (Z - bed), of a wet cell (0 if none is wet) */
	uint64_t max_depth_cell;     /* flat ids y * cols + x in the LOCAL array; ties go to the lowest id; UINT64_MAX if none */
	uint64_t max_speed_cell;
} hp_domain_stats_t;
int hp_domain_stats(hp_domain_t* d, int64_t row0, int64_t nrows, hp_domain_stats_t* out);   /* BLOCKS */

/* ---- the peak tracker: run-long maps a final state cannot give (no reference counterpart; closest: the Zmax field,
 *      CLSchemeGodunov.clc, the one run-long quantity the flux kernels carry because the reference does).
 *      Opt-in.  A set of fp64 accumulator rasters in device memory (8 bytes per cell and enabled value) into which one kernel
 *      folds the current state each time the host asks for a sample.  The maxima are maxima over the SAMPLES, not over the
 *      iterations: the host chooses the cadence, and a sample is only ever taken between batches (inside hp_step_batch every
 *      iteration but the last carries its successor's rain, and an iteration pair never materialises its middle state).  A
 *      sample reads the buffer hp_domain_download(HP_ARRAY_STATE) reads and the device's own "Time" scalar, in stream order
 *      behind whatever is queued, without any host synchronisation, and changes nothing the steps depend on: a tracked run's
 *      trajectory is the untracked run's, bit for bit.  With tracking off nothing is allocated or launched.
 *      Conventions of the output stage: all arithmetic in fp64 whatever the domain's precision (an fp32 domain's values are
 *      widened first), correctly rounded operations only (add, multiply, divide, square root, compare), NODATA = -9999,
 *      depth = Z - bed, wet = depth > 1e-8, v = sqrt((Qx / depth)^2 + (Qy / depth)^2).  A cell is counted exactly as in
 *      hp_domain_stats (Zmax > -9999 and bed <= 9999); a sample changes only cells that are counted and wet in it, so cells
 *      that are never counted stay NODATA in every value.
 *        HP_PEAK_SPEED           largest v over the samples in which the cell was wet; NODATA if never wet
 *        HP_PEAK_UNIT_DISCHARGE  largest sqrt(Qx^2 + Qy^2) over those samples
 *        HP_PEAK_HAZARD          largest depth * (v + 0.5) over those samples (the DEFRA/EA FD2320 rating without the debris term)
 *        HP_PEAK_ARRIVAL_TIME    model time of the first sample with depth > arrival_depth; NODATA if none
 *        HP_PEAK_WET_DURATION    sum of (t_sample - t_previous_sample) over the samples with depth > arrival_depth (right-endpoint
 *                                rule), added in sample order; NODATA if none.  The first sample's t_previous is the device time at
 *                                hp_peaks_enable / hp_peaks_reset; samples at a suspended sync point repeat the time and add 0. ---- */
enum { HP_PEAK_SPEED = 0, HP_PEAK_UNIT_DISCHARGE = 1, HP_PEAK_HAZARD = 2, HP_PEAK_ARRIVAL_TIME = 3, HP_PEAK_WET_DURATION = 4,
       HP_PEAK_COUNT = 5 };
typedef struct {
	uint32_t struct_size;        /* = sizeof(hp_peaks_desc_t) */
	uint32_t values_mask;        /* bit v: HP_PEAK_* value v is tracked; at least one, none beyond HP_PEAK_COUNT */
	double   arrival_depth;      /* metres; at least 1e-8 (a cell that is dry in a sample changes nothing).  Typical: 0.01 */
} hp_peaks_desc_t;
/* Allocates the accumulators of values_mask (and only those) and resets them; on a domain that is already tracking, the old set
 * is freed first.  If the allocation fails the call returns HP_ERR_HIP and the domain stays usable with tracking off. */
int hp_peaks_enable(hp_domain_t* d, const hp_peaks_desc_t* desc);
int hp_peaks_disable(hp_domain_t* d);                  /* frees; idempotent (also done by hp_domain_destroy) */
/* NODATA everywhere, sample count 0, t_previous = the device time now; enqueued.  hp_domain_upload does not touch the peaks:
 * a host that replaces the state resets them itself if it wants to. */
int hp_peaks_reset(hp_domain_t* d);
/* One sample: enqueued on the domain's stream, never blocks.  HP_ERR_STATE before hp_peaks_enable and between hp_step_begin
 * and hp_step_end. */
int hp_peaks_sample(hp_domain_t* d);
/* hp_domain_derive's contract: rasters[i] receives value values[i] (each at most once, each one of the enabled ones) for rows
 * [row0, row0 + nrows) of the LOCAL array, element_bytes 8 (the accumulators: a plain device-to-host copy) or 4 (those values
 * rounded once, through the output stage's bounded scratch in blocks of rows).  Reads in stream order behind the queued
 * samples; the host memory must stay alive until hp_sync().  Argument errors are HP_ERR_INVALID before any device call,
 * a read before hp_peaks_enable or inside a split step is HP_ERR_STATE; nrows == 0 is HP_OK. */
int hp_peaks_read(hp_domain_t* d, const int* values, int count, int element_bytes,
                  void* const* rasters, int64_t row0, int64_t nrows);
/* Samples taken since enable / reset and the model times of the first and the last of them (both the time at enable / reset
 * while there is none).  Any of the three pointers may be NULL.  BLOCKS. */
int hp_peaks_info(hp_domain_t* d, uint64_t* samples, double* t_first, double* t_last);

/* ---- the probe recorder: time series at gauge cells and through cross-sections ("probes" = gauges + sections;
 *      no reference counterpart: HiPIMS-OCL writes rasters only, and a hydrograph from it means a raster per sample).
 *      Opt-in.  One kernel launch per sample (csrc/hp_probes.hpp: record_probes) writes one RECORD of
 *      stride = 1 + 4 * gauge_count + section_count fp64 words into a buffer of `capacity` records in device memory:
 *          [t, g0.z, g0.depth, g0.qx, g0.qy, g1.z, ..., s0.discharge, s1.discharge, ...]
 *      A sample reads the buffer hp_domain_download(HP_ARRAY_STATE) reads, the bed and the device's own "Time" scalar, in stream
 *      order behind whatever is queued, without any host synchronisation, and changes nothing the steps depend on: a recorded
 *      run's state, scalars, launch counts and pair statistics are the unrecorded run's, bit for bit.  With the recorder off
 *      nothing is allocated or launched.  A sample can only be taken between batches, never per iteration inside one: inside
 *      hp_step_batch every iteration but the last carries its successor's rain, and an iteration pair never materialises its
 *      middle state -- there is no state "at iteration k" to read (the peak tracker's rule).
 *      Conventions of the output stage: all arithmetic in fp64 whatever the domain's precision (an fp32 domain's values are
 *      widened first), correctly rounded add, multiply and compare only, NODATA = -9999, wet = Z - bed > 1e-8.  A cell is counted
 *      exactly as in hp_domain_stats (Zmax > -9999 and bed <= 9999).
 *        gauge     counted: z = Z, depth = Z - bed (raw: not clamped, no wet test), qx = Qx, qy = Qy (m2/s); not counted: NODATA
 *                  in all four.  The same cell may be listed more than once.
 *        section   a list of m >= 2 cells with one weight pair (wx, wy) in {-1, 0, 1} each.  The term of entry k is
 *                  (double)wx_k * Qx_k + (double)wy_k * Qy_k (two multiplies, one add, not fused) if its cell is counted and wet,
 *                  +0.0 otherwise.  THE ORDER OF THE SUM IS PART OF THE CONTRACT: 256 partial sums, partial j = +0.0 + term_j +
 *                  term_(j+256) + term_(j+512) + ... in that order; then for s = 128, 64, ..., 1: part[i] = part[i] + part[i+s]
 *                  for i < s (the halving tree of hp_domain_stats); discharge = dx * part[0] in m3/s, one multiply.  No atomics:
 *                  the same state gives the same bits, on any launch shape, and frontend.ProbeRecorder restates it in NumPy.
 *                  A cell may appear more than once in a section. ---- */
typedef struct {
	uint32_t struct_size;              /* = sizeof(hp_probes_desc_t) */
	uint32_t capacity;                 /* samples the device buffer holds; >= 1; capacity * stride * 8 <= 256 MiB */
	uint64_t gauge_count;              /* <= 65536 */
	const uint64_t* gauge_cells;       /* flat ids y * cols + x in the LOCAL array */
	uint32_t section_count;            /* <= 1024; gauge_count + section_count >= 1 */
	const uint64_t* section_offsets;   /* section_count + 1 entries into the three arrays below, from 0; each section >= 2 entries */
	const uint64_t* section_cells;     /* LOCAL flat ids */
	const int8_t*   section_wx;        /* -1, 0, 1 */
	const int8_t*   section_wy;
} hp_probes_desc_t;
/* Copies the lists to the device (the caller's arrays are free again on return) and allocates the record buffer; sample count 0.
 * On a domain that is already recording, the old recorder is freed first.  Argument errors -- a bad struct_size, a cell id
 * >= cols * rows, a weight outside {-1, 0, 1}, a section shorter than 2 entries, a count over its limit, a record buffer over
 * 256 MiB -- are HP_ERR_INVALID before any device call.  If an allocation fails the call returns HP_ERR_HIP and the domain
 * stays usable with the recorder off. */
int hp_probes_enable(hp_domain_t* d, const hp_probes_desc_t* desc);
int hp_probes_disable(hp_domain_t* d);                 /* frees; idempotent (also done by hp_domain_destroy) */
/* Sample count 0; the buffer is not cleared.  Reads queued before the call still deliver the old records (stream order). */
int hp_probes_reset(hp_domain_t* d);
/* One sample: enqueued on the domain's stream, never blocks.  HP_ERR_STATE before hp_probes_enable, between hp_step_begin and
 * hp_step_end, and when samples == capacity: nothing is enqueued then and the count is unchanged -- the host reads the records
 * and calls hp_probes_reset. */
int hp_probes_sample(hp_domain_t* d);
/* Records [first, first + count) into records[count * stride]: a device-to-host copy enqueued behind the queued samples; the host
 * memory must stay alive until hp_sync().  first + count beyond the samples taken is HP_ERR_INVALID; a read before
 * hp_probes_enable or inside a split step is HP_ERR_STATE; count == 0 is HP_OK. */
int hp_probes_read(hp_domain_t* d, uint64_t first, uint64_t count, double* records);
/* Samples taken since enable / reset, the capacity and the record stride in fp64 words.  Host-side counters: does not block.  Any
 * of the three pointers may be NULL.  HP_ERR_STATE before hp_probes_enable. */
int hp_probes_info(hp_domain_t* d, uint64_t* samples, uint64_t* capacity, uint64_t* stride);

/* ---- the zone recorder: per-zone cell counts, volume of water, largest depth and speed as a time series (a zone = the cells that
 *      carry one id in a 2-byte raster: a sub-catchment, a ward, a reservoir; no reference counterpart: HiPIMS-OCL writes rasters
 *      only).  Rasters, peaks, points and lines have their observers above; this one answers for AREAS, and with one zone over the
 *      whole grid it is a mass-balance series that does not block, which hp_domain_stats cannot give.
 *      Opt-in.  One fill and one kernel launch per sample (csrc/hp_zones.hpp: record_zones) write one RECORD of
 *      stride = 1 + 7 * zone_count 64-bit words into a buffer of `capacity` records in device memory:
 *          [t | zone 1: cells, cells_wet, cells_flooded, depth_hi, depth_lo, max_depth, max_speed | zone 2: ... ]
 *      Word 0 is the bit pattern of the device's own "Time" scalar as fp64.  A sample reads the buffer
 *      hp_domain_download(HP_ARRAY_STATE) reads, the bed and that scalar, in stream order behind whatever is queued, without any
 *      host synchronisation, and changes nothing the steps depend on: a recorded run's state, scalars, launch counts and pair
 *      statistics are the unrecorded run's, bit for bit.  With the recorder off nothing is allocated or launched.  A sample can
 *      only be taken between batches (the peak tracker's rule).
 *      Conventions of the output stage: values widened to fp64 first whatever the domain's precision, correctly rounded
 *      operations only (add, multiply, divide, square root, round to integer, compare).  A cell is counted exactly as in
 *      hp_domain_stats (Zmax > -9999 and bed <= 9999).  depth = Z - bed; d = depth > 0 ? depth : 0, then at most 1048576.0.
 *      Per zone, over the counted cells that carry its id:
 *        0 cells          counted cells
 *        1 cells_wet      depth > 1e-8
 *        2 cells_flooded  depth > flood_depth
 *        3 depth_hi       sum of (q >> 32), q = (uint64) rint(d * 4294967296.0): round half to even; the scaling is exact, q <= 2^52
 *        4 depth_lo       sum of (q & 0xffffffff).  The exact sum is S = depth_hi * 2^32 + depth_lo; the zone's volume is
 *                         dx^2 * S / 2^32: the quantum is 2^-32 m and the error at most 2^-33 m per cell
 *        5 max_depth      bit pattern of the largest d (non-negative doubles order like their bit patterns); 0 without a counted cell
 *        6 max_speed      bit pattern of the largest sp = sqrt((Qx / depth)^2 + (Qy / depth)^2) over the wet cells with sp > 0 (a NaN
 *                         or a zero speed contributes nothing); 0 if no cell qualifies
 *      ALL SEVEN ARE SUMS OR MAXIMA OF INTEGERS: the record is a pure function of the state and the id raster -- independent of
 *      the launch shape, of the order in which the atomics arrive and of how the grid is cut into strips.  The records of an
 *      N-strip run (ghost rows carrying id 0), words added and maxima taken, are the single domain's in every bit;
 *      frontend.ZoneRecorder restates the record in NumPy and frontend.combine_zones the combination.  Cells with id 0 contribute
 *      nothing; a zone that no cell carries stays all-zero. ---- */
enum { HP_ZONE_WORDS = 7 };
typedef struct {
	uint32_t struct_size;              /* = sizeof(hp_zones_desc_t) */
	uint32_t capacity;                 /* records the device buffer holds; >= 1; capacity * stride * 8 <= 256 MiB */
	uint32_t zone_count;               /* 1 .. 4096 */
	uint32_t reserved;
	const uint16_t* zone_of_cell;      /* cols * rows ids of the LOCAL array, row 0 = south; 0 = in no zone, 1..zone_count */
	double   flood_depth;              /* metres, >= 1e-8: the "flooded" threshold.  Typical: 0.1 */
} hp_zones_desc_t;
/* Copies the id raster to the device (2 bytes per cell there too; the caller's array is free again on return) and allocates the
 * record buffer; sample count 0.  On a domain that is already recording, the old recorder is freed first.  Argument errors -- a
 * bad struct_size, a NULL pointer, zone_count outside 1..4096, flood_depth below 1e-8, a record buffer over 256 MiB, an id above
 * zone_count (the message names the first such cell) -- are HP_ERR_INVALID before any device call.  If an allocation fails the
 * call returns HP_ERR_HIP and the domain stays usable with the recorder off. */
int hp_zones_enable(hp_domain_t* d, const hp_zones_desc_t* desc);
int hp_zones_disable(hp_domain_t* d);                  /* frees; idempotent (also done by hp_domain_destroy) */
/* Sample count 0; the buffer is not cleared.  Reads queued before the call still deliver the old records (stream order). */
int hp_zones_reset(hp_domain_t* d);
/* One sample: enqueued on the domain's stream, never blocks.  HP_ERR_STATE before hp_zones_enable, between hp_step_begin and
 * hp_step_end, and when samples == capacity: nothing is enqueued then and the count is unchanged -- the host reads the records
 * and calls hp_zones_reset. */
int hp_zones_sample(hp_domain_t* d);
/* Records [first, first + count) into records[count * stride]: a device-to-host copy enqueued behind the queued samples; the host
 * memory must stay alive until hp_sync().  first + count beyond the samples taken is HP_ERR_INVALID; a read before
 * hp_zones_enable or inside a split step is HP_ERR_STATE; count == 0 is HP_OK. */
int hp_zones_read(hp_domain_t* d, uint64_t first, uint64_t count, uint64_t* records);
/* Samples taken since enable / reset, the capacity and the record stride in 64-bit words.  Host-side counters: does not block.
 * Any of the three pointers may be NULL.  HP_ERR_STATE before hp_zones_enable. */
int hp_zones_info(hp_domain_t* d, uint64_t* samples, uint64_t* capacity, uint64_t* stride);

/* ---- the moving bed: time-varying breaches and barriers (no reference counterpart: its bed is loaded once,
 *      CDomainCartesian::loadInitialConditions, Domain/Cartesian/CDomainCartesian.cpp:163-283).  Every other forcing of the engine is
 *      a source term; this one moves the terrain: an embankment that fails over twenty minutes, a barrier that closes at a given
 *      time, a defence that goes in stages.  Opt-in.  A SHAPE is a list of cells, one target elevation per cell and one progress
 *      series {time, fraction} shared by the shape's cells.  hp_bed_apply evaluates every shape's fraction from the device's own
 *      "Time" scalar, in stream order behind whatever is queued, without any host synchronisation, and moves the bed of the listed
 *      cells; the host calls it between batches (never inside one: the peak tracker's rule).
 *      THE CONTRACT: an apply is exactly the host round trip it replaces -- hp_domain_download of state and bed, the bed moved and the
 *      levels shifted on the host (frontend.BedShapes.apply restates it in NumPy), hp_domain_upload(HP_ARRAY_BED),
 *      hp_domain_upload(HP_ARRAY_STATE) -- in every bit of the state, the bed and the scalars of the run that follows, with
 *      iteration pairs, STRICT arithmetic and strips included.  A domain without shapes, or one that never applies, queues exactly
 *      what it queues without this block.
 *        Fraction.  All arithmetic in fp64, correctly rounded multiply, add, divide and compare only, never fused.  With t the
 *      "Time" scalar widened and the series (t_0, f_0) ... (t_last, f_last): t <= t_0 gives f_0; t >= t_last gives f_last; otherwise,
 *      in the segment with t_k <= t < t_k+1, f = f_k + (f_k+1 - f_k) * ((t - t_k) / (t_k+1 - t_k)), in that order.  Fractions
 *      need not be monotone: a gate reopens.
 *        New bed of a listed cell.  base = the cell's bed when its shape was added.  f <= 0 gives base; f >= 1 gives target
 *      (base + (target - base) need not be target); otherwise base + f * (target - base).  Rounded once to the domain's
 *      precision: b1.
 *        The apply.  A listed cell is skipped if it is not counted in the sense of hp_domain_stats (Zmax > -9999 and bed <= 9999
 *      counts) or if b1 equals its stored bed b0.  For every other listed cell, with the values of the buffer
 *      hp_domain_download(HP_ARRAY_STATE) reads widened to fp64 and every result rounded once on store:
 *      Z1 = b1 + (Z0 - b0) (the depth is kept raw: no clamp, no wet test), Zmax1 = Zmax0 > Z1 ? Zmax0 : Z1, Qx and Qy unchanged,
 *      bed = b1.  Then both ping-pong buffers hold the patched state and the engine forgets what an upload of bed and state makes
 *      it forget (the cost: one device-to-device copy of the whole state per apply). ---- */
typedef struct {
	uint32_t struct_size;              /* = sizeof(hp_bed_shape_desc_t) */
	uint32_t series_entries;           /* 1 .. 4096 */
	uint64_t cell_count;               /* >= 1; all shapes of a domain together <= 1048576 */
	const uint64_t* cells;             /* flat ids y * cols + x in the GLOBAL grid, as hp_boundary_add_cell */
	const double*   target;            /* cell_count elevations, finite, |target| <= 9999 */
	const double*   series;            /* series_entries x {time, fraction}: times strictly increasing, fractions in [0, 1] */
} hp_bed_shape_desc_t;
typedef struct {
	uint32_t struct_size;              /* = sizeof(hp_bed_info_t), set by the caller */
	uint32_t shapes;                   /* shapes on the domain */
	uint64_t cells_local;              /* listed cells this domain (strip) keeps */
	uint64_t applies;                  /* applies queued since the first shape was added (hp_bed_shapes_clear starts over) */
	uint64_t changed_last;             /* cells the last apply changed (skipped cells do not count); 0 before the first */
	uint64_t changed_total;            /* ... and all applies together */
	double   t_last;                   /* the device time the last apply saw; 0 before the first */
} hp_bed_info_t;
/* Adds a shape (at most 64).  Copies the lists to the device (the caller's arrays are free again on return) and captures
 * base[k] = bed[cell_k] with a gather on the domain's stream: the bed is not read back to the host.  A strip keeps the cells whose
 * row lies in its local array, ghost rows included, and drops the others silently: every rank adds every shape with global ids.
 * A cell may be listed at most once over all shapes of a domain (the message names the first repeated id).  A LATER
 * hp_domain_upload(HP_ARRAY_BED) TOUCHES NEITHER THE SHAPES NOR THEIR base: a host that replaces the bed clears the shapes and adds
 * them again.  Argument errors -- a bad struct_size, a NULL pointer, a count over its limit, a target that is not finite or beyond
 * 9999, a time that is not finite or does not increase, a fraction outside [0, 1] or NaN, a repeated cell, an id at or above
 * cols * global_rows -- are HP_ERR_INVALID before any device call; between hp_step_begin and hp_step_end the call returns
 * HP_ERR_STATE.  If an allocation fails the call returns HP_ERR_HIP and the domain stays usable with the shapes it had. */
int hp_bed_shape_add(hp_domain_t* d, const hp_bed_shape_desc_t* desc);
int hp_bed_shapes_clear(hp_domain_t* d);               /* frees; idempotent (also done by hp_domain_destroy) */
/* One apply: one kernel launch over the listed cells (csrc/hp_bed.hpp: bed_apply), then what the two uploads do.  Enqueued on the
 * domain's stream, never blocks.  With no shape on the domain: HP_OK, nothing is enqueued.  HP_ERR_STATE between hp_step_begin
 * and hp_step_end, and on a strip whose ghost rows are not all valid (two reaches of ghost rows after an odd number of iterations:
 * apply after an even batch). */
int hp_bed_apply(hp_domain_t* d);
int hp_bed_info(hp_domain_t* d, hp_bed_info_t* out);   /* BLOCKS */

/* Device-side checkpoint: what saveCurrentState + rollbackSimulation do through host memory (CSchemeGodunov.cpp:1720-1736,
 * :1474-1518), kept in HBM instead (two more copies of a 4096^2 fp64 state are 1 GB of 288).  hp_state_save copies BOTH
 * ping-pong buffers and the time-control block; hp_state_restore puts each buffer, the time-control block, the ping-pong phase
 * and the remembered CFL maxima back: the steps that follow repeat the original ones bit for bit.  (The reference's rollback
 * writes the saved next-source state into both buffers; cells whose whole neighbourhood is dry, which the flux kernel leaves
 * untouched -- quirk Q3 --, then continue from other values than in the original run.  A host that wants exactly that uploads
 * the state it downloaded, as CSchemeMI::rollbackSimulation does.)  The host may then adjust time / target / timestep with the calls
 * below, exactly as the reference's rollback sequence does.
 * While the peak tracker is on, hp_state_save also snapshots its accumulators and its own block and hp_state_restore puts
 * them back: the samples that follow repeat the original ones bit for bit.  A snapshot taken before the tracker was enabled,
 * disabled or re-enabled holds no peaks: hp_state_restore then resets them and sends one HP_LOG_WARNING to the log sink.
 * While the probe recorder is on, hp_state_save remembers its sample count and hp_state_restore puts it back: the records taken
 * since then are re-recorded by the samples that are repeated.  If the recorder was enabled, disabled, re-enabled or reset since
 * the snapshot, hp_state_restore sets the count to 0 and sends one HP_LOG_WARNING to the log sink.  The zone recorder's sample
 * count follows the same rule, with a warning of its own.
 * While the domain has bed shapes, hp_state_save also keeps the bed at the listed cells (hp_state_restore brings back neither the
 * bed nor the boundary list, and a roll-back across an hp_bed_apply would leave levels of one bed over another) and
 * hp_state_restore puts it back.  If shapes were added or cleared since the snapshot, hp_state_restore leaves the bed as it is
 * and sends one HP_LOG_WARNING to the log sink.
 * While the domain has link groups (hp_boundary_add_links), hp_state_save also keeps the links' records and hp_state_restore puts
 * them back: the iterations that are repeated count again what they counted.  If link groups were added or cleared since the
 * snapshot, hp_state_restore sets the records of the links the domain has now to zero and sends one HP_LOG_WARNING to the log
 * sink: the probe recorder's rule.
 * While the domain has an infiltration (hp_boundary_add_infiltration), hp_state_save also copies F and hp_state_restore puts it
 * back.  If the infiltration was added or cleared since the snapshot, hp_state_restore leaves F as it is and sends one
 * HP_LOG_WARNING to the log sink.
 * While the domain has a tracer (hp_tracer_enable), hp_state_save also copies the current M with its phase and iteration counter
 * and hp_state_restore puts them back, by the infiltration's rule. */
int hp_state_save(hp_domain_t* d);
int hp_state_restore(hp_domain_t* d);

/* ---- boundaries: CBoundaryUniform / CBoundaryGridded::prepareBoundary
 *      (Boundaries/CBoundaryUniform.cpp:180-296, CBoundaryGridded.cpp:166-300); the arrays are the packed
 *      buffers those functions build.  Applied in the order added (the reference's order is unspecified, Q7) */
enum { HP_UNIFORM_RAIN_INTENSITY = 0, HP_UNIFORM_LOSS_RATE = 1 };           /* Boundaries/CLBoundaries.clh:44-45 */
enum { HP_GRIDDED_RAIN_INTENSITY = 0, HP_GRIDDED_RAIN_ACCUMUL = 1, HP_GRIDDED_MASS_FLUX = 2 };   /* :47-50 */
/* series: `entries` x {time, value} pairs (value in mm/h), element type = domain precision */
int hp_boundary_add_uniform(hp_domain_t* d, int definition, const void* series, uint32_t entries,
                            double interval, double length);
/* grids: [entries][grid_rows][grid_cols] rates (mm/h), element type = domain precision.  A cell (x, gy) reads column
 * floor((x dx - offset_x) / resolution) and row floor((gy dx - offset_y) / resolution) of the grid, evaluated in the domain's
 * precision.  A grid that does not cover every interior cell (0 <= column < grid_cols, 0 <= row < grid_rows at columns
 * 1 .. cols - 2 and global rows 1 .. global_rows - 2) is HP_ERR_INVALID, "gridded boundary does not cover the domain's
 * interior cells": the cover check is made in the domain's precision, with the kernels' own expression, so an fp32 domain
 * can refuse a grid that an fp64 domain of the same shape takes (the float quotient can reach grid_cols where the double
 * one stays just below).  The offsets are therefore at most dx. */
int hp_boundary_add_gridded(hp_domain_t* d, int definition, const void* grids, uint64_t entries,
                            uint64_t grid_rows, uint64_t grid_cols, double resolution,
                            double offset_x, double offset_y, double interval);
/* CBoundaryCell::prepareBoundary (Boundaries/CBoundaryCell.cpp:300-445) -- "next" row N2 of SURVEY.md 8(f).
 * cells: flat ids y*cols + x in the GLOBAL grid (CDomainCartesian::getCellID); series: `entries` x {time, depth or
 * level, Qx, Qy}, already divided by the cell count for "total" discharges as the reference's packer does (:398-402). */
enum { HP_DEPTH_IGNORE = 0, HP_DEPTH_IS_FSL = 1, HP_DEPTH_IS_DEPTH = 2, HP_DEPTH_IS_CRITICAL = 3 };       /* CLBoundaries.clh:34-37 */
enum { HP_DISCHARGE_IGNORE = 0, HP_DISCHARGE_IS_DISCHARGE = 1, HP_DISCHARGE_IS_VELOCITY = 2, HP_DISCHARGE_IS_VOLUME = 3 };   /* :39-42 */
int hp_boundary_add_cell(hp_domain_t* d, int depth_definition, int discharge_definition, const uint64_t* cells,
                         uint64_t count, const void* series, uint64_t entries, double interval, double length);
/* ---- link groups: water passes THROUGH an embankment -- a culvert under a road, a weir into a storage basin, a flap-valved
 *      outfall, a pumping station behind a defence (no reference counterpart: the reference moves water between face neighbours and
 *      in and out of the model through prescribed sources only).  A LINK joins two cells a and b, anywhere in the grid, and moves
 *      water between them as a function of their OWN levels; a link group is the fourth boundary kind, next to uniform, gridded and
 *      cell: applied once per iteration on the iteration's source buffer, at its place in the order added, like a cell boundary.
 *      The kernel is one thread per link (csrc/hp_links.hpp: bdy_links): a cell is an end of at most one link over all groups of a
 *      domain, so it needs no atomics and does not depend on any order.
 *      A domain with a link group is not fusable (hp_boundaries_fused is false, as with a cell boundary), so it runs single
 *      iterations, never iteration pairs; and it never runs a speculative STRICT batch (a batch that is queued again would count
 *      the records twice).  Under MUSCL-Hancock links are inert, like every boundary (quirk Q8).
 *      THE CONTRACT.  All arithmetic in fp64 whatever the domain's precision, the stored values widened first; correctly rounded
 *      add, multiply, divide, square root and compare only, never fused; each stored level is rounded once.  dt is the "Timestep"
 *      scalar, dx the cell size as the kernels hold it (rounded to the domain's precision), g the engine's own constant (9.81).
 *      Per link and iteration:
 *        1. Inert cases.  The link is inert if dt <= 0 or if either end is not counted in the sense of hp_domain_stats (a cell is
 *      counted when Zmax > -9999 and bed <= 9999).  An inert link sets q_last = +0.0 and changes nothing else.
 *        2. Direction.  up = a if Za >= Zb, else b; dn the other end.  A pump always has up = a.  If one_way is set and up == b,
 *      Q = 0.
 *        3. Discharge Q in m3/s.  Weir: hu = Zup - level; Q = 0 unless hu > 0, otherwise Q = ((coeff * size) * hu) * sqrt(hu), and
 *      with hd = Zdn - level, if hd > limit * hu then Q = Q * sqrt((hu - hd) / (hu * (1 - limit))).  Orifice: Q = 0 unless
 *      Zup > level, otherwise dH = Zup - max(Zdn, level) and Q = min((coeff * size) * sqrt((2 * g) * dH), limit).  Pump: Q = size if
 *      Za > level, else 0.
 *        4. Level change.  dz = (Q * dt) / (dx * dx).  avail = Zup - max(level, bed_up): if !(avail > 0) then dz = 0, else
 *      dz = min(dz, avail).  For weir and orifice also dz = min(dz, 0.5 * (Zup - Zdn)): a link cannot overshoot equal levels.
 *        5. Stores.  If dz > 0: Zup = Zup - dz and Zdn = Zdn + dz.  Zmax, Qx and Qy are left as they are, as a cell boundary
 *      leaves Zmax.
 *        6. Record.  With s = +1 for a -> b (up == a) and -1 otherwise: q_last = s * ((dz * (dx * dx)) / dt);
 *      volume = volume + s * (dz * (dx * dx)), one add per iteration, in iteration order; active += (dz > 0).
 *      frontend.Links restates all of it in NumPy; tests/links_probe.cpp holds the two to each other bit for bit.
 *      TWO THINGS TO KNOW.  A link acts on the source buffer only.  If it drains its upstream cell while that cell's whole
 *      neighbourhood is dry, the flux kernel leaves the cell untouched in the OTHER ping-pong buffer, as the reference does with
 *      every such cell (quirk Q3): the level the cell had two iterations earlier comes back with the next iteration and is passed on
 *      once more.  A pump that empties an isolated polder therefore moves more than the polder held; keep such a cell's
 *      neighbourhood wet or give the pump a switch-on level above the bed.  And the products of finite parameters must be finite:
 *      coeff * size that overflows is an argument error (with dH == 0 it would leave a NaN in `volume` for good).
 *      STRIPS.  Every rank adds every group with GLOBAL ids.  A strip must store both ends of a link, ghost rows included, or
 *      neither: storing exactly one end is HP_ERR_UNSUPPORTED, and the message names the link.  A strip with two reaches of ghost
 *      rows holds its outermost reach on every second iteration only: an end on such a row with the other end on a row that is
 *      always valid is refused in the same way.  Two strips that both store a link compute the same bits redundantly; a link's
 *      record is the one held by the strip that owns a. ---- */
enum { HP_LINK_WEIR = 0, HP_LINK_ORIFICE = 1, HP_LINK_PUMP = 2 };
typedef struct {
	uint64_t cell_a, cell_b;           /* flat ids y * cols + x in the GLOBAL grid, as hp_boundary_add_cell; both interior */
	int32_t  kind;                     /* HP_LINK_* */
	int32_t  one_way;                  /* != 0: a -> b only (flap valve) */
	double   level;                    /* weir: crest elevation; orifice: invert; pump: switch-on level at a */
	double   size;                     /* weir: crest width, m; orifice: flow area, m2; pump: rate, m3/s (always a -> b) */
	double   coeff;                    /* weir: m^0.5/s; orifice: dimensionless; pump: ignored */
	double   limit;                    /* weir: modular limit in [0, 1); orifice: discharge cap, m3/s (+inf for none); pump: ignored */
} hp_link_t;
typedef struct {
	double   q_last;                   /* the discharge the last iteration realised, m3/s, a -> b positive */
	double   volume;                   /* what has passed since the group was added, m3, a -> b positive */
	uint64_t active;                   /* iterations in which the link moved water */
	uint64_t reserved;
} hp_link_record_t;
/* Adds one link group (at most 65536 links over all groups of a domain).  Both cells of a link must be interior: not within the
 * scheme's reach of the grid's ring (the ring test of hp_boundary_add_cell; a ring cell is rejected, not flagged), and a cell may be
 * an end of at most one link over all groups of the domain (the message names the first repeated id).  Argument errors -- a NULL
 * pointer, count 0 or over the limit, an unknown kind, a level, size, coeff or coeff * size that is not finite, a negative size or coeff, a limit
 * outside its range or NaN, a == b, a ring cell, a repeated cell, an id at or above cols * global_rows -- are HP_ERR_INVALID before
 * any device call; between hp_step_begin and hp_step_end the call returns HP_ERR_STATE. */
int hp_boundary_add_links(hp_domain_t* d, const hp_link_t* links, uint64_t count);
/* Records first .. first + count - 1, in the order the links were added over all groups.  Enqueued; valid after hp_sync (the host
 * memory must stay alive until then).  first + count beyond the domain's links is HP_ERR_INVALID; count == 0 is HP_OK. */
int hp_links_read(hp_domain_t* d, uint64_t first, uint64_t count, hp_link_record_t* out);
int hp_links_info(hp_domain_t* d, uint64_t* links, uint64_t* groups);   /* host counters; either pointer may be NULL */
/* ---- infiltration: water leaves the surface into the soil -- Green-Ampt by soil class (no reference counterpart: the reference
 *      takes water out through the uniform loss rate only, one number for the whole domain and no memory).  Every cell carries a
 *      soil class id (0 = impervious) and its cumulative infiltrated depth F; the infiltration is the fifth boundary kind, next to
 *      uniform, gridded, cell and link groups: applied once per iteration on the iteration's source buffer, at its place in the
 *      order added.  The kernel is one lane per cell (csrc/hp_soil.hpp: bdy_infiltration): a streaming pass over the class bytes
 *      that touches the state and F only where the class is not 0.
 *      STATE.  One fp64 raster F in device memory (8 bytes per cell) and one byte per cell for the class id; nothing of either
 *      exists on a domain that never adds infiltration, and such a domain queues exactly what it queued without this call.
 *      At most one infiltration per domain: a second hp_boundary_add_infiltration is HP_ERR_STATE.  A domain with it is not
 *      fusable (hp_boundaries_fused is false, as with a cell boundary or a link group), so it runs single iterations, never
 *      iteration pairs; and it never runs a speculative STRICT batch (a batch that is queued again would add to F twice).  Under
 *      MUSCL-Hancock it is inert, like every boundary (quirk Q8): F does not move.
 *      THE CONTRACT.  All arithmetic in fp64 whatever the domain's precision, the stored values widened first; correctly rounded
 *      add, multiply, divide, square root and compare only, never fused.  dt is the "Timestep" scalar; S = suction * deficit is
 *      formed once on the host.  Per cell and iteration:
 *        1. The cell is untouched, F included, if dt <= 0, if its class is 0, if it is not counted in the sense of
 *      hp_domain_stats (a cell is counted when Zmax > -9999 and bed <= 9999), or if it lies on the edge ring of the GLOBAL grid
 *      (column 0 or cols - 1, global row 0 or global_rows - 1): the area boundaries' rule.  The flux kernels never write the ring
 *      and the engine prices the ring's part of the timestep once per upload, so nothing drains it.
 *        2. depth = Z - bed.  If !(depth > 0), nothing happens.
 *        3. The potential: the closed-form Green-Ampt step of CASC2D / GSSHA, finite at F == 0.  kd = ks * dt;
 *      b = kd - 2.0 * F; disc = b * b + (8.0 * kd) * (S + F); pot = 0.5 * (b + sqrt(disc)).  If !(pot > 0), pot = 0.
 *        4. room = capacity - F.  If !(room > 0), pot = 0; else if room < pot, pot = room.
 *        5. dF = depth < pot ? depth : pot.
 *        6. If dF > 0: Z = (T)(Z - dF), rounded once, and F = F + dF.  Zmax, Qx and Qy stay as they are: the loss rate's and the
 *      links' rule.  A cell with dF == 0 is not stored at all.
 *      frontend.Infiltration restates all of it in NumPy; tests/soil_probe.cpp holds the two to each other bit for bit.
 *      STRIPS.  The id raster and `initial` are of the LOCAL array, ghost rows included, as the zone raster is.  Every strip
 *      recomputes F on its ghost rows: F is a function of the cell's own history of (Z, dt), and with an exchange after every
 *      iteration that history is its owner's bit for bit, so nothing of F is exchanged.  A strip with two reaches of ghost rows
 *      holds its outermost reach on every second iteration only, and F there would drift from its owner's: on such a strip
 *      hp_boundary_add_infiltration returns HP_ERR_UNSUPPORTED. ---- */
typedef struct {
	double ks;                         /* saturated hydraulic conductivity, m/s; finite, >= 0 */
	double suction;                    /* wetting-front suction head psi, m; finite, >= 0 */
	double deficit;                    /* moisture deficit dtheta, -; in [0, 1] */
	double capacity;                   /* largest cumulative infiltration, m; >= 0, +inf for none */
} hp_soil_class_t;
typedef struct {
	uint32_t struct_size;
	uint32_t class_count;              /* 1..255 */
	const hp_soil_class_t* classes;    /* class k is classes[k-1] */
	const uint8_t* soil_of_cell;       /* cols*rows ids of the LOCAL array, row 0 = south; 0 = impervious, 1..class_count */
	const double*  initial;            /* cols*rows cumulative infiltration F0 in m (finite, >= 0), or NULL for zeros: a hot start */
} hp_infiltration_desc_t;
/* Argument errors -- a bad struct_size, a NULL pointer, class_count outside 1..255, an id above class_count, a non-finite or
 * negative ks or suction, a deficit outside [0, 1], a NaN or negative capacity, a non-finite ks * 1e6 or suction * deficit, a
 * negative or non-finite initial -- are HP_ERR_INVALID before any device call; where a cell is at fault the message names the
 * first offending cell.  Between hp_step_begin and hp_step_end the call returns HP_ERR_STATE.  If an allocation fails the call
 * returns HP_ERR_HIP and the domain stays usable without infiltration.  The arrays are free on return. */
int hp_boundary_add_infiltration(hp_domain_t* d, const hp_infiltration_desc_t* desc);
/* Rows row0 .. row0 + nrows - 1 of F (fp64, cols values a row).  Enqueued; valid after hp_sync (the host memory must stay alive
 * until then).  A row range outside the array is HP_ERR_INVALID; a domain without infiltration, or a call between hp_step_begin
 * and hp_step_end, HP_ERR_STATE. */
int hp_infiltration_read(hp_domain_t* d, double* raster, int64_t row0, int64_t nrows);
/* Host counters, does not block: the classes of the domain's infiltration and its cells of a class other than 0 (both 0 without
 * one); either pointer may be NULL. */
int hp_infiltration_info(hp_domain_t* d, uint32_t* classes, uint64_t* pervious_cells);
/* ---- the open boundary: water LEAVES the model -- the downstream edge of a catchment, the seaward side of an estuary (no reference
 *      counterpart: the reference's edges are closed walls or never-written cells).  An open boundary is a set of SEGMENTS of the
 *      grid's edge ring; it is the sixth boundary kind, next to uniform, gridded, cell, link groups and the infiltration: applied once
 *      per iteration on the iteration's source buffer, at its place in the order added.  Every ring cell of a segment takes the depth
 *      and the outward momentum of its inward neighbour -- a zero-gradient, outflow-only edge -- and records the discharge that leaves
 *      through its face.  The kernel is one lane per listed ring cell (csrc/hp_open.hpp: bdy_open): a ring cell is in at most one
 *      segment of the domain, so it needs no atomics and does not depend on any order.
 *      A domain that never calls hp_boundary_add_open allocates nothing and queues exactly what it queued without this call.  A
 *      domain with an open boundary is not fusable (hp_boundaries_fused is false, as with a cell boundary), so it runs single
 *      iterations, never iteration pairs; and it never runs a speculative STRICT batch (a batch that is queued again would add to
 *      `volume` twice).  The ring's part of the timestep is priced anew on every iteration, as with a cell boundary on ring cells.
 *      THE CONTRACT.  All arithmetic in fp64 whatever the domain's precision, the stored values widened first; correctly rounded add,
 *      subtract, multiply and compare only, never fused; each stored value is rounded once to the domain's precision T.  dt is the
 *      "Timestep" scalar, dx the cell size as the kernels hold it (rounded to T and widened).  r is the ring cell, i its inward
 *      neighbour (the cell next to it across the edge's face), n the state component normal to the edge (Qx for west / east, Qy for
 *      south / north), s the other one.  Per listed ring cell and iteration:
 *        1. Inert.  The cell is inert if dt <= 0, or if r or i is not counted in the sense of hp_domain_stats (a cell is counted when
 *      Zmax > -9999 and bed <= 9999): a closed-edge wall inside a segment is simply inert.  An inert cell sets q_last = +0.0 and
 *      changes nothing else.
 *        2. Depth.  d = Z_i - bed_i.  If !(d > 0) then d = 0.
 *        3. Level.  lvl = bed_r + d.  If lvl > Z_i then lvl = Z_i > bed_r ? Z_i : bed_r: the ring never stands above the water that
 *      feeds it, and nothing runs in downhill from outside.
 *        4. Momentum.  If d == 0 then Qn = Qs = +0.0.  Otherwise Qs = Qs_i, and Qn = Qn_i if it points out of the grid (> 0 on east
 *      and north, < 0 on west and south), else Qn = +0.0.
 *        5. Stores.  Z_r = (T)lvl; Zmax_r = Zmax_r > Z_r ? Zmax_r : Z_r; Qx and Qy as above.
 *        6. Record.  F is the first component (the mass flux) of the exact face solve between i and the ring cell as just stored: the
 *      STRICT make_side / face_solve of csrc/hp_math.hpp in the domain's precision whatever the domain's math_mode, with the argument
 *      order the flux kernel uses for that face of i (the tracer's rule: one arithmetic, not two).  out = +F on east and north, -F on
 *      west and south.  q_last = out * dx; volume = volume + (out * dt) * dx, one add per iteration, in iteration order;
 *      active += (out > 0).
 *      WHAT THE RECORD IS.  The face flux that the flux launch that follows uses for cell i -- in the exact arithmetic; a FAST domain's
 *      own flux differs from it by that mode's tolerance.  It is not i's realised loss: the flux kernel zeroes net changes below the dry
 *      threshold and snaps nearly dry cells to the bed, so the sum of the records and the water that left the interior differ by at
 *      most a few dry thresholds per cell and iteration.
 *      frontend.Open restates all of it in NumPy; tests/open_probe.cpp holds the two to each other bit for bit.
 *      STRIPS.  Every rank adds every segment with GLOBAL indices.  A strip keeps the ring cells whose row lies in its local array,
 *      ghost rows included; west and east cells on ghost rows are recomputed redundantly (their inward neighbour lies in the same row
 *      and is valid with one reach of ghost rows).  A cell's record is the one held by the strip that owns its row.  A strip with two
 *      reaches of ghost rows holds its outermost reach on every second iteration only, and the records there would drift from their
 *      owners': on such a strip hp_boundary_add_open returns HP_ERR_UNSUPPORTED (the infiltration's rule and reason). ---- */
enum { HP_EDGE_SOUTH = 0, HP_EDGE_NORTH = 1, HP_EDGE_WEST = 2, HP_EDGE_EAST = 3 };
typedef struct {
	int32_t edge;                      /* HP_EDGE_* */
	int32_t reserved;                  /* 0 */
	int64_t first, last;               /* inclusive, along the edge in the GLOBAL grid: the column x for south and north, the global row for
	                                      west and east; both in 1 .. n - 2 (the four corner cells touch no interior cell) */
} hp_open_segment_t;
typedef struct {
	double   q_last;                   /* the discharge through the cell's face in the last iteration, m3/s, outward positive */
	double   volume;                   /* what has passed since the segment was added, m3, outward positive */
	uint64_t active;                   /* iterations in which water left through the face */
	uint64_t reserved;
} hp_open_record_t;
/* Adds `count` segments (at most 64 over the domain).  Records are ordered by segment in the order added, and by ascending index
 * inside a segment.  Argument errors -- a NULL pointer, count 0, more than 64 segments on the domain, an unknown edge, a non-zero
 * `reserved`, first > last, an index outside 1 .. n - 2, a ring cell listed twice over all segments of the domain -- are
 * HP_ERR_INVALID before any device call, and the message names the segment and the first offending cell; between hp_step_begin and
 * hp_step_end the call returns HP_ERR_STATE.  HP_ERR_UNSUPPORTED, with the reason in the message: a scheme other than Godunov (the
 * record is the Godunov face flux; under MUSCL-Hancock every boundary is inert anyway, quirk Q8), and a strip with two reaches of ghost
 * rows. */
int hp_boundary_add_open(hp_domain_t* d, const hp_open_segment_t* segments, uint32_t count);
/* Records first .. first + count - 1.  Enqueued; valid after hp_sync (the host memory must stay alive until then).  first + count
 * beyond the domain's listed ring cells is HP_ERR_INVALID; count == 0 is HP_OK. */
int hp_open_read(hp_domain_t* d, uint64_t first, uint64_t count, hp_open_record_t* out);
int hp_open_info(hp_domain_t* d, uint32_t* segments, uint64_t* cells);   /* host counters (cells: of the GLOBAL grid); either pointer may be NULL */
/* hp_state_save / hp_state_restore keep and restore the open boundary's records by the links' rule: if segments were added or cleared
 * since the snapshot, the restore zeroes the records and sends one HP_LOG_WARNING. */
int hp_boundary_clear(hp_domain_t* d);                 /* removes link groups too (and their records), the infiltration with its F, and the open boundary with its records */
/* Are the domain's area boundaries carried by the flux kernel itself (rain / loss of iteration n+1 added to the state
 * iteration n stores, no separate pass over the grid)?  True for the Godunov scheme with up to three uniform / gridded
 * boundaries, no cell boundary among them, and rain grids of at least 64 model cells per grid cell; everything else runs
 * the boundary kernels as separate launches like the reference (CSchemeGodunov.cpp:1637-1643).  Results are identical
 * either way; bench.py reports it. */
int hp_boundaries_fused(hp_domain_t* d, int* fused);

/* ---- the passive tracer: a solute carried with the water (no reference counterpart: the reference moves water only).  It answers
 *      where water came from and where something dissolved in it goes: a spill at an outfall, the share of river water in a
 *      basement.  The stored quantity is a MASS PER UNIT AREA M (units * m: concentration x depth), not a concentration: rain
 *      dilutes it without touching it, the sum of M over a closed domain is conserved to rounding, and a cell that dries keeps
 *      its residue.
 *      STATE.  Two fp64 rasters of the local array in device memory (the old and the new M, 16 bytes per cell) with a phase of
 *      their own, independent of the state's ping-pong buffers, whatever the domain's precision.  Nothing of it exists on a
 *      domain that never calls hp_tracer_enable, and such a domain queues exactly what it queued without these calls.  A domain
 *      with it is not fusable (hp_boundaries_fused is false), runs single iterations, never iteration pairs, and never runs a
 *      speculative STRICT batch (a batch queued again would move M twice).
 *      THE STEP.  Once per iteration, behind EVERY boundary of the list whatever the order added and in front of the flux
 *      launch: the kernel (csrc/hp_tracer.hpp: tracer_step, one lane per cell) reads the source buffer the flux kernel is about
 *      to read and the "Timestep" scalar dt before the flux launch advances it, and writes only M.  T is the domain's precision.
 *        0. Sources first (tracer_sources): if dt > 0, M += (rate(t) * dt) / (dx * dx) at each listed cell, rate the source's
 *      {time, mass rate} series at the device's "Time" scalar by the bed shapes' rule (hp_bed_shape_add: the first value at or
 *      before the first time, the last at or after the last, r_k + (r_k+1 - r_k) * ((t - t_k) / (t_k+1 - t_k)) in between), all
 *      of it in fp64.
 *        1. Copy cases, M' = M: a ring cell (column 0 or cols - 1, row 0 or rows - 1: the cells the flux kernel never writes);
 *      any cell when dt <= 0; a disabled cell (Zmax <= -9999 or Z == -9999); a cell for which Z - bed < dry_threshold (in T)
 *      holds in the cell and in its four neighbours (quirk Q3's condition, under which no water moves).
 *        2. The four face mass fluxes FN, FS, FE, FW exactly as the flux kernel's exact arithmetic forms them: the first
 *      component of the HLLC flux behind the reconstruction, same argument order, in precision T -- the STRICT face solve
 *      WHATEVER the domain's math_mode: the tracer's arithmetic is one thing, not two.
 *        3. Everything below in fp64, the values widened first; correctly rounded add, multiply, divide and compare only, never
 *      fused.  h_k = (double)Z_k - (double)bed_k from the RAW source state, not the reconstructed one;
 *      c_k = h_k > 1e-10 ? M_k / h_k : 0, for the cell (C) and its four neighbours.
 *        4. Each face takes the concentration of the cell the water leaves: GE = FE > 0 ? FE * cC : FE * cE;
 *      GW = FW > 0 ? FW * cW : FW * cC; GN = FN > 0 ? FN * cC : FN * cN; GS = FS > 0 ? FS * cS : FS * cC.
 *        5. M' = M - dt * (((GE - GW) + (GN - GS)) / dx), in this order, dx as the kernels hold it (rounded to T, widened).
 *      There is no clamp and no limiter.  The two cells of a face take the same upwind concentration, so what one loses the
 *      other gains, up to the rounding of the face flux as each of the two forms it and of the final M - dt * (...).  A face
 *      whose neighbour is a copy case still carries its flux; a wall gives F = 0 by the reconstruction.
 *      frontend.Tracer restates all of it in NumPy; tests/tracer_probe.cpp holds steps 0 and 3 to 5 to it bit for bit.
 *      WHAT IT SAYS ABOUT THE WATER.  The flux kernel zeroes net changes below the dry threshold and snaps nearly dry cells to
 *      the bed, and in FAST arithmetic its fluxes differ from the STRICT ones in the last bits: so M / h can leave
 *      [min c, max c] by rounding-sized amounts and at drying fronts, while M itself stays conserved.  The uniform loss rate
 *      takes water and leaves M (evaporation).  hp_bed_apply keeps the depth and so leaves M alone.
 *      REFUSED, HP_ERR_UNSUPPORTED, with the reason in the message: a scheme other than Godunov; a strip
 *      (global_rows != rows: M's ghost rows would need an exchange of their own); a domain with link groups or an infiltration
 *      (both move water that would have to carry M) -- and hp_boundary_add_links / hp_boundary_add_infiltration on a traced
 *      domain likewise.
 *      hp_domain_upload does not touch M; hp_boundary_clear does not touch the tracer; hp_domain_destroy frees it.
 *      hp_state_save / hp_state_restore carry the current M, its phase and the iteration counter; if the tracer was enabled or
 *      disabled since the snapshot, hp_state_restore leaves M as it is and sends one HP_LOG_WARNING to the log sink. ---- */
typedef struct {
	uint32_t struct_size;
	uint32_t reserved;                 /* 0 */
	const double* initial;             /* cols*rows M0 of the LOCAL array in units * m (finite, >= 0), row 0 = south, or NULL for zeros */
} hp_tracer_desc_t;
/* Argument errors -- a NULL desc, a bad struct_size, a negative or non-finite initial (the message names the first bad cell) --
 * are HP_ERR_INVALID before any device call.  Between hp_step_begin and hp_step_end the call returns HP_ERR_STATE, as does a
 * second enable.  If an allocation fails the call returns HP_ERR_HIP and the domain stays usable without a tracer.  `initial`
 * is free on return. */
int hp_tracer_enable(hp_domain_t* d, const hp_tracer_desc_t* desc);
int hp_tracer_disable(hp_domain_t* d);                 /* frees M and the sources; idempotent (also done by hp_domain_destroy) */
/* One source: `count` cells (flat ids of the grid, y * cols + x) that each receive the mass rate of `series` (`entries` pairs
 * {time in s, rate in units per second}, times finite and strictly increasing, rates finite; a negative rate takes mass out).
 * Argument errors -- a NULL pointer, entries outside 1..4096, count outside 1..1048576, a cell outside the grid, on the edge
 * ring or listed twice over all sources, more than 64 sources or 1 048 576 cells in all -- are HP_ERR_INVALID before any device
 * call; HP_ERR_STATE before hp_tracer_enable and between hp_step_begin and hp_step_end.  The arrays are free on return. */
int hp_tracer_add_source(hp_domain_t* d, const uint64_t* cells, uint64_t count, const double* series, uint32_t entries);
int hp_tracer_sources_clear(hp_domain_t* d);
/* Rows row0 .. row0 + nrows - 1 of the current M (fp64, cols values a row).  Enqueued; valid after hp_sync (the host memory must
 * stay alive until then).  A NULL raster or a row range outside the array is HP_ERR_INVALID; a domain without a tracer, or a
 * call between hp_step_begin and hp_step_end, HP_ERR_STATE; nrows == 0 is HP_OK. */
int hp_tracer_read(hp_domain_t* d, double* raster, int64_t row0, int64_t nrows);
/* ... and the reverse: the rows of the current M are replaced (the values are the caller's: no check).  The raster is free on return. */
int hp_tracer_write(hp_domain_t* d, const double* raster, int64_t row0, int64_t nrows);
/* Host counters, does not block: the iterations the tracer has been stepped through since hp_tracer_enable (as restored by
 * hp_state_restore), its sources and their cells (all 0 without a tracer); any pointer may be NULL. */
int hp_tracer_info(hp_domain_t* d, uint64_t* iterations, uint32_t* sources, uint64_t* source_cells);

/* ---- a tracer SET: K species carried in one pass, each with a first-order decay.  Separating river, rain and sewer water, or a
 *      spill from a background load, takes one run of the water, not K: the face mass fluxes depend on the water only, so one
 *      kernel launch per iteration (csrc/hp_tracer.hpp: tracer_step_set) forms the copy-case verdict and FN, FS, FE, FW of a cell
 *      once and moves every species by them.  A domain has at most ONE tracer, single (hp_tracer_enable) or set; a second enable
 *      of either form is HP_ERR_STATE.  Everything the tracer block above says holds per species: the state (two allocations of
 *      K * cols * rows doubles, the old and the new planes, species after species, with one phase for the whole set), the place
 *      in the iteration, steps 0 to 5 word for word -- the STRICT face solve whatever the math mode, the copy cases --, what it
 *      does to the water's launches, and what is refused: hp_tracer_enable_set refuses exactly what hp_tracer_enable refuses, for
 *      the same reasons, and hp_boundary_add_links / hp_boundary_add_infiltration refuse a domain with a set likewise.
 *        6. Decay, after step 5 and in fp64, correctly rounded multiply, add and divide only, never fused, at EVERY cell of the
 *      array, copy cases and ring included: M'' = (lambda_s > 0 && dt > 0) ? M' / (1.0 + lambda_s * dt) : M'.  Implicit Euler: it
 *      never overshoots zero and is stable for any dt; residue on dry ground decays too.  With lambda_s == 0 nothing is divided.
 *      THE BITS.  Species s of a set equals, in every bit of M after every iteration, a single tracer (hp_tracer_enable) on the
 *      same water with that species' initial raster and sources if lambda_s == 0, and frontend.Tracer(decay=lambda_s) -- K of
 *      them are frontend.TracerSet -- for any lambda_s.  State, scalars, launch counts and pair statistics of the run are those of
 *      the single-tracer run.  hp_tracer_enable_set always runs tracer_step_set, K == 1 included; hp_tracer_enable keeps
 *      tracer_step.
 *      SOURCES feed one species each; a cell may be listed once PER SPECIES over that species' sources; the limits on sources
 *      (64) and listed cells (1 048 576) hold over the whole set.
 *      THE SINGLE-TRACER CALLS ON A SET: hp_tracer_add_source, hp_tracer_read and hp_tracer_write act on species 0;
 *      hp_tracer_disable frees all species; hp_tracer_info counts sources and cells over all species; hp_tracer_sources_clear
 *      clears all sources.  The per-species calls on a single tracer see a set of one species.
 *      hp_state_save / hp_state_restore carry all K current planes, the phase and the iteration counter by the tracer's rule;
 *      enabling, disabling or changing K since the snapshot is the stale case: M is left as it is, one HP_LOG_WARNING. ---- */
#define HP_TRACER_MAX_SPECIES 8
typedef struct {
	uint32_t struct_size;
	uint32_t species;                  /* K, 1..8 */
	const double* decay;               /* K rates lambda in 1/s, finite and >= 0, or NULL for zeros */
	const double* initial;             /* K planes of cols*rows M0 (finite, >= 0), species after species, or NULL for zeros */
} hp_tracer_set_desc_t;
/* Argument errors -- a NULL desc, a bad struct_size, species outside 1..8, a negative or non-finite decay rate (the message names
 * the species) or initial value (species and cell) -- are HP_ERR_INVALID before any device call; HP_ERR_STATE, HP_ERR_HIP and
 * HP_ERR_UNSUPPORTED as hp_tracer_enable.  The arrays are free on return. */
int hp_tracer_enable_set(hp_domain_t* d, const hp_tracer_set_desc_t* desc);
/* hp_tracer_add_source for species `species`; a species >= K is HP_ERR_INVALID before any device call. */
int hp_tracer_add_source_to(hp_domain_t* d, uint32_t species, const uint64_t* cells, uint64_t count, const double* series, uint32_t entries);
/* hp_tracer_read / hp_tracer_write on the current plane of species `species`; a species >= K is HP_ERR_INVALID. */
int hp_tracer_read_species(hp_domain_t* d, uint32_t species, double* raster, int64_t row0, int64_t nrows);
int hp_tracer_write_species(hp_domain_t* d, uint32_t species, const double* raster, int64_t row0, int64_t nrows);
/* Host values, does not block: K (0 without a tracer, 1 for a single one) and the K decay rates into decay[0 .. K - 1] (an array
 * of HP_TRACER_MAX_SPECIES doubles); either pointer may be NULL. */
int hp_tracer_set_info(hp_domain_t* d, uint32_t* species, double* decay);

/* ---- exchange with the bed: a species of a tracer set may settle onto the ground and be picked up again.  A decay rate destroys
 *      mass; silt, sediment-bound metals and sewage solids do not vanish: they drop out where the water slows, lie on the ground
 *      and are entrained again by the next flood wave.  A species of a set (hp_tracer_enable_set) can exchange mass with a DEPOSIT
 *      D: a second fp64 raster per species, in M's units (units * m, mass per unit area), that lies on the ground: it does not move,
 *      does not decay and is not diluted.  Opt-in per species by hp_tracer_set_exchange; the bed itself does not change.
 *        7. Exchange, after step 6, for every species with settling > 0 || erodibility > 0, in the same launch
 *      (csrc/hp_tracer.hpp: tracer_step_set<T, true>, tracer_exchange), ONLY at cells that are not copy cases of step 1 (ring cells,
 *      dt <= 0, disabled cells, five dry cells: those keep M'' and D).  Everything in fp64 on widened values, by correctly
 *      rounded add, multiply, divide and compare and the correctly rounded cube root of csrc/hp_crmath.h, never fused, in this order:
 *          h = (double)Z - (double)bed of the iteration's raw source state (step 3's h); if !(h > 1e-10) nothing happens.
 *          vx = Qx / h; vy = Qy / h; sp2 = vx*vx + vy*vy;
 *          n: the Manning value the flux kernel uses for the cell (the uniform value or the array's element), widened;
 *          nn = n*n; tau = ((9810.0 * nn) * sp2) / hp_cr_cbrt(h);            rho g n^2 |u|^2 / h^(1/3), N/m2
 *          deposition (Krone) if settling > 0 && M'' > 0 && tau < tau_deposit:
 *              pd = tau_deposit == +inf ? 1.0 : 1.0 - tau / tau_deposit;  k = (settling * pd) * dt;  r = k / h;
 *              M3 = M'' / (1.0 + r);  dep = M'' - M3;  D = D + dep;  M = M3;                       implicit Euler, as the decay
 *          else erosion (Partheniades) if erodibility > 0 && D > 0 && tau > tau_erode:
 *              ex = tau / tau_erode - 1.0;  ero = (erodibility * ex) * dt;  if (ero > D) ero = D;  D = D - ero;  M = M'' + ero;
 *      A NaN tau fails both comparisons; tau_erode >= tau_deposit makes the branches exclusive.  M + D of a species changes by
 *      rounding only in this step: with lambda == 0 a closed domain conserves the sum of M and D.
 *      THE BITS.  Every plane of M and D equals frontend.TracerSet(exchange=...) in every bit after every iteration, whatever the
 *      math mode.  A set without an exchanging species, and every other path, queues exactly what it queued before
 *      (tracer_step_set<T, false>); a single tracer (hp_tracer_enable) keeps tracer_step.
 *      STORAGE.  D is K planes of cols * rows doubles, allocated by the first successful hp_tracer_set_exchange of the domain;
 *      planes of species without exchange stay zero and are never touched.  D is updated in place.  hp_tracer_disable and
 *      hp_domain_destroy free it; hp_domain_upload and hp_boundary_clear do not touch it.
 *      hp_state_save / hp_state_restore carry D in the tracer's own copy, behind M.  The FIRST hp_tracer_set_exchange of a domain
 *      counts as a change of the store: a snapshot taken before it is the tracer's stale case (M and D are left as they are, one
 *      HP_LOG_WARNING).  A later call, for the same or another species, changes parameters (and D's plane if deposit_initial is
 *      given) only and stales nothing. ---- */
typedef struct {
	uint32_t struct_size;
	uint32_t species;                  /* < K */
	double   settling;                 /* w_s, m/s: finite, >= 0; 0 = never deposits */
	double   tau_deposit;              /* tau_cd, N/m2: > 0, +inf allowed (= deposits at any shear, probability 1) */
	double   tau_erode;                /* tau_ce, N/m2: >= tau_deposit, +inf allowed (= never erodes) */
	double   erodibility;              /* E, units/(m2 s): finite, >= 0; 0 = never erodes */
	const double* deposit_initial;     /* cols*rows D0 of the LOCAL array (finite, >= 0) or NULL: zeros on the first call for the domain, keep D on a later one */
} hp_tracer_exchange_desc_t;
/* Argument errors -- a NULL desc, a bad struct_size, species >= K, a settling, tau_deposit, tau_erode (also < tau_deposit) or
 * erodibility outside its range (the message names the field), a negative or non-finite deposit_initial (the message names the first
 * bad cell) -- are HP_ERR_INVALID before any device call.  HP_ERR_STATE before a tracer exists and between hp_step_begin and
 * hp_step_end; HP_ERR_UNSUPPORTED on a single tracer from hp_tracer_enable (enable it as a set of one); HP_ERR_HIP if D cannot be
 * allocated: the domain stays usable without exchange.  The raster is free on return. */
int hp_tracer_set_exchange(hp_domain_t* d, const hp_tracer_exchange_desc_t* desc);
/* hp_tracer_read_species / hp_tracer_write_species on the plane of D of species `species`; HP_ERR_STATE while no species exchanges. */
int hp_tracer_deposit_read (hp_domain_t* d, uint32_t species, double* raster, int64_t row0, int64_t nrows);
int hp_tracer_deposit_write(hp_domain_t* d, uint32_t species, const double* raster, int64_t row0, int64_t nrows);
/* Host values, does not block: the number of species with settling > 0 || erodibility > 0, and what was set for each of the K species
 * into out[0 .. K - 1] (struct_size and species filled in, pointers NULL; a species never set: 0, +inf, +inf, 0); either may be NULL. */
int hp_tracer_exchange_info(hp_domain_t* d, uint32_t* exchanging_species, hp_tracer_exchange_desc_t out[HP_TRACER_MAX_SPECIES]);

/* ---- time control ---- */
int hp_set_target_time(hp_domain_t* d, double t);     /* CScheme::setTargetTime -> "Target time (sync)" buffer (:1166-1176) */
int hp_set_time(hp_domain_t* d, double t);            /* rewrite the "Time" buffer: rollbackSimulation (:1480-1494) */
int hp_force_timestep(hp_domain_t* d, double dt);     /* CSchemeGodunov::forceTimestep (:1803-1811) + write (:1213-1232) */
int hp_reset_counters(hp_domain_t* d);                /* tst_ResetCounters (CLDynamicTimestep.clc:151-161) */
int hp_update_timestep(hp_domain_t* d);               /* tst_Reduce + tst_UpdateTimestep (:1189-1195, :1254-1260) */

/* ---- the hot loop: `n` x CScheme*::scheduleIteration (CSchemeGodunov.cpp:1617-1666,
 *      CSchemeMUSCLHancock.cpp:646-680), enqueued without blocking ---- */
int hp_step_batch(hp_domain_t* d, uint32_t n_iterations);

typedef struct {
	double   time;               /* "Time" buffer */
	double   timestep;           /* "Timestep" buffer; negative = suspended at the sync point */
	double   time_hydrological;
	double   time_target;
	double   batch_timesteps;    /* "Batch timesteps cumulative" */
	uint32_t batch_successful;   /* "Batch successful iterations" */
	uint32_t batch_skipped;      /* "Batch skipped iterations" */
	uint64_t cells_calculated;   /* ulCurrentCellsCalculated: cols*rows per queued iteration (:1299) */
	uint64_t iterations;
} hp_scalars_t;

/* CSchemeGodunov::readKeyStatistics (:1817-1835) after the five queueReadAll calls (:1309-1313); BLOCKS */
int hp_read_scalars(hp_domain_t* d, hp_scalars_t* out);
int hp_sync(hp_domain_t* d);                          /* COCLDevice::blockUntilFinished */
/* COCLDevice::isBusy.  With HP_STRICT_SPECULATE=1 the call that finds a speculative batch finished also looks at its verdict
 * and may re-queue the batch with the plain divisions: *busy is then 1 again (the call may ENQUEUE work; it never blocks on it). */
int hp_is_busy(hp_domain_t* d, int* busy);
/* Inside a batch an iteration is one launch whose last block waits for the flux blocks' maxima and advances the time.  That wait
 * is bounded (HP_TAIL_TIMEOUT_MS, environment, default 20000): a block that never reports -- only possible if blocks were ever
 * dispatched out of order -- freezes time and timestep instead of hanging the GPU, and hp_sync / hp_read_scalars and every later
 * call on the domain fail with HP_ERR_STATE.  (No reference counterpart: its queue is a sequence of separate kernels.) */

/* ---- multi-GPU strips (one process per GPU).  The engine never talks to other ranks itself: the host
 *      moves ghost rows and the wave-speed maximum with its collective library (RCCL through
 *      torch.distributed in this repo) on the domain's stream, between these calls.  Replaces
 *      CDomainLink::pullFromBuffer/pushToBuffer + CMPIManager (MPI/CMPIManager.cpp:555-709, :852-861). ---- */
/* Split form of one iteration: boundaries + flux kernel (+ local CFL maximum) ... */
int hp_step_begin(hp_domain_t* d);
/* ... then, after the host has all-reduced (MAX) the 8-byte value at hp_device_ptr(HP_PTR_CFL_MAX),
 * the time advance (tst_Advance_Normal) and the ping-pong flip. */
int hp_step_end(hp_domain_t* d);
/* Between hp_step_begin and hp_step_end: does this iteration carry a NEW local maximum that has to be all-reduced?
 * (0 on iterations whose reduction re-reads an unchanged buffer -- quirk Q1 -- and in fixed-timestep mode.) */
int hp_step_needs_reduction(hp_domain_t* d, int* needed);

enum {
	HP_PTR_STATE_NEXT_SRC = 0,   /* state buffer the next iteration reads (ghost rows are written here) */
	HP_PTR_STATE_OTHER    = 1,
	HP_PTR_BED            = 2,
	HP_PTR_MANNING        = 3,
	HP_PTR_CFL_MAX        = 4,   /* one element of the domain precision: local max wave speed */
	HP_PTR_SCALARS        = 5
};
int hp_device_ptr(hp_domain_t* d, int which, void** ptr);
int hp_stream(hp_domain_t* d, void** hip_stream);     /* the domain's hipStream_t (COCLDevice's command queue) */
/* Halo overlap.  When on, hp_step_begin runs the row segments that hold the rows the strip neighbours need
 * (the first/last owned rows) on a second, higher-priority stream and the interior segments on the domain's
 * stream; the domain's stream joins the second one before anything that follows (CFL maximum, hp_step_end).  The
 * host starts its halo send/recv on hp_stream_halo right after hp_step_begin -- ordered after the halo rows only,
 * so the transfer overlaps the interior compute -- and makes the domain's stream wait for the transfer before
 * hp_step_end.  Results are identical either way.  Replaces the reference's overlap-by-wide-ghost-zones scheme
 * (CDomainLink.cpp:297-328), which exists to amortise host-staged copies.  Off by default. */
int hp_set_halo_overlap(hp_domain_t* d, int on);
int hp_stream_halo(hp_domain_t* d, void** hip_stream);

/* ---- the strip loop driven from C++ (one process per GPU).  The per-iteration protocol above -- flux launches, ghost
 *      rows to and from the two strip neighbours, all-reduce(MAX) of the wave speed, time advance -- queued by the
 *      library itself on RCCL, so that a C++ host (HiPIMS's CModel / CMPIManager) needs no collective code of its own and
 *      the host cost per iteration is a handful of enqueues.  Replaces CDomainLink::pullFromBuffer / pushToBuffer
 *      (Domain/Links/CDomainLink.cpp:168-270) and CMPIManager's block exchange and MPI_Allreduce(MIN)
 *      (MPI/CMPIManager.cpp:555-709, :852-861).  Ranks are ordered south to north: rank k's neighbours are k-1 and k+1.
 *      The collective library is loaded at run time (dlopen): pass the copy the process already uses (a torch process:
 *      torch/lib/librccl.so), or NULL for the system's.  The unique id is created on rank 0 and handed to the other
 *      ranks by the host's own means (MPI_Bcast in HiPIMS, a torch broadcast in this repository's tests). ---- */
#define HP_COMM_ID_BYTES 128
int hp_comm_load(const char* rccl_library_path);   /* a path is tried alone; NULL tries librccl.so, librccl.so.1, /opt/rocm/lib/librccl.so */
int hp_comm_unique_id(void* id_out /* HP_COMM_ID_BYTES */);
int hp_strip_comm_init(hp_domain_t* d, const void* id, int rank, int world);   /* collective: every rank calls it; turns the halo overlap on unless hp_set_halo_overlap chose */
int hp_strip_step_batch(hp_domain_t* d, uint32_t n_iterations);               /* hp_step_batch for a strip */
int hp_strip_update_timestep(hp_domain_t* d);                                 /* hp_update_timestep for a strip (collective) */
int hp_strip_comm_destroy(hp_domain_t* d);
/* What the strip loop is really running on (reporting: bench.py puts it into its JSON line).  `library` is the file the
 * dynamic loader resolved the collective library to, `comm_ranks` the rank count that library reports for the domain's
 * communicator (ncclCommCount; -1 without a communicator).  d == NULL: library path only.  No reference counterpart
 * (CMPIManager logs its node count, MPI/CMPIManager.cpp:63-80). */
typedef struct {
	char    library[256];
	int32_t comm_ranks;
	int32_t comm_rank;
	int32_t halo_overlap;        /* 1: halo rows on their own stream, the transfer overlaps the interior launch */
	int32_t ghost_rows;          /* ghost rows per interior side: the stencil reach (exchange every iteration) or twice that (every second) */
	int32_t peer_max;            /* 1: the maximum over the strips travels through peer-written mailboxes, 0: through the library's all-reduce */
	int32_t peer_halo;           /* 1: the ghost rows are written by the strips into each other's state buffers, 0: sent and received through the library */
} hp_strip_info_t;
int hp_strip_info(hp_domain_t* d, hp_strip_info_t* out);

/* ---- the maximum over all strips without a collective ("one-shot all-gather-to-all over direct links, then a
 * local max"; stands where MPI_Allreduce(MIN dt) is, MPI/CMPIManager.cpp:852-861) ----
 * Every strip owns a small mailbox in uncached device memory which the other strips' GPUs write directly over xGMI; the
 * advance kernel that runs after every flux launch anyway (or the flux launch's own tail block) stores its maximum into every peer's mailbox, waits for theirs
 * and folds them -- no collective kernel on the critical path of an iteration.
 *   hp_strip_peer_ticket   allocates the mailbox and describes it and the domain's two state buffers (addresses for ranks
 *                          of the same process, IPC handles for other processes) in HP_PEER_TICKET_BYTES that the host
 *                          hands to every rank by its own means, like the communicator id;
 *   hp_strip_peer_connect  takes all ranks' tickets in rank order (count <= 64), maps the peers' mailboxes and the strip
 *                          neighbours' state buffers and runs a connection test (two reductions with known answers,
 *                          bounded wait).  COLLECTIVE.  With a communicator the ranks then agree (one all-reduce) on what
 *                          ALL of them can do:
 *                            *active = 2  mailboxes and ghost rows: hp_strip_step_batch runs ONE launch per iteration and calls
 *                                         nothing of the collective library inside an iteration -- the tiles that compute the
 *                                         strip's edge rows store them into the neighbours' ghost rows as well (CDomainLink's
 *                                         push / pull, Domain/Links/CDomainLink.cpp:168-270), and the launch's tail block
 *                                         holds the mailbox round, on every iteration, which is the hand-over;
 *                            *active = 1  mailboxes only (a rank could not map a neighbour's buffers, or HP_PEER_DIRECT=0
 *                                         in some rank's environment): the rows keep going through ncclSend / ncclRecv;
 *                            *active = 0  nothing: everything stays with the library (the reason goes to the log sink as
 *                                         a warning; the call still returns HP_OK).
 *                          Without a communicator (diagnostic use) *active is this rank's own verdict on its mailboxes;
 *   hp_strip_peer_round    one reduction of a caller-given value (diagnostic; COLLECTIVE over the connected ranks);
 *   hp_strip_peer_disconnect  unmaps and frees (also done by hp_strip_comm_destroy and hp_domain_destroy).
 * A strip that is not heard from within HP_PEER_TIMEOUT_MS (environment, default 10000) raises a sticky error instead of
 * hanging the GPU: hp_read_scalars then fails with HP_ERR_HIP. */
#define HP_PEER_TICKET_BYTES 384
int hp_strip_peer_ticket(hp_domain_t* d, void* ticket_out);
int hp_strip_peer_connect(hp_domain_t* d, const void* tickets, int count, int rank, int* active);
int hp_strip_peer_round(hp_domain_t* d, double value, double* max_out);
int hp_strip_peer_disconnect(hp_domain_t* d);

/* ---- measurement hooks (no reference counterpart; COCLDevice has no profiling queue, COCLDevice.cpp:283-288) ----
 * Bracket a region of the domain's stream with HIP events and return the elapsed milliseconds. */
int hp_timer_start(hp_domain_t* d);
int hp_timer_stop(hp_domain_t* d, float* elapsed_ms);  /* BLOCKS until the stop event completes */
/* Average device time of the dominant (flux) kernel: every `stride`-th launch is bracketed with events from a pool of
 * 16 pairs created by this call (so nothing is created inside a timed region); sampling stops when the pool is used up.
 * The time an EMPTY event pair takes (measured by this call on the idle stream) is taken off every sample. */
int hp_kernel_timing(hp_domain_t* d, int enable_stride);
int hp_kernel_timing_read(hp_domain_t* d, double* avg_ms, uint32_t* samples);   /* BLOCKS */
/* The cost of an empty event pair that the last hp_kernel_timing() measured and hp_kernel_timing_read() takes off every
 * sample (raw average = avg_ms + this): reported so that lines with and without the correction can be compared. */
int hp_kernel_timing_overhead(hp_domain_t* d, double* overhead_ms);
/* Iteration PAIRS.  Where it is the same computation -- Godunov scheme, the tuned kernel, quirk Q1 on, no boundary conditions or only
 * area boundaries the flux kernel can carry (hp_boundaries_fused), a grid of about a round of blocks and more -- hp_step_batch runs two
 * iterations as ONE launch (hp_kernels.hpp: godunov_march2; half the HBM traffic).  Everything observable through this interface is what
 * single iterations leave, with ONE condition in FAST arithmetic: a cell the reference leaves untouched at a pair's first step (quirk Q3,
 * CLSchemeGodunov.clc:248-255) passes its current state on where the reference keeps the stale one of the iteration before -- different
 * only if the cell dried out that very step.  The EXACT flavour writes those stale values down between launches (4-9 % slower) and runs
 * where they matter: STRICT arithmetic always, domains whose boundaries remove water (loss rate, mass flux), and on request.
 *   HP_TWO_STEP=0 / 1    pairs off / on wherever eligible (default: by grid size; STRICT: by the engine's own measurement, the two being
 *                        the same bits)                    HP_PAIR_EXACT=0 / 1   the exact flavour nowhere / everywhere
 *   HP_PAIR_BDY=0        domains with area boundaries keep single iterations      HP_PAIR_STRICT=0   so does STRICT arithmetic
 *   HP_PAIR_SKIP=0       FAST fp64 pairs keep no still records and skip no tiles (the same bits; A/B runs)
 *   HP_PAIR_WALL=0       ... keep them, but march the still water in the windows next to the edge ring (the same bits; A/B runs)
 *   HP_PAIR_ORDER=0      the same launches start their tiles tile-row by tile-row, not the column groups that marched last time first
 *                        (the same bits; A/B runs)
 * hp_launch_counts and hp_pair_stats show what ran. */
/* How many whole-domain flux launches the domain has queued since it was created, and how many of them carried their own tail
 * block (reduction + time advance inside the flux launch: an iteration is then ONE launch; otherwise the flux launch is followed
 * by an advance launch).  bench.py states its roofline basis from the difference of two readings around the timed region. */
int hp_launch_counts(hp_domain_t* d, uint64_t* flux_launches, uint64_t* with_tail);

/* Diagnostics of the iteration pairs, for tests and A/B runs; blocks (a stream synchronisation; the stamps are counted by a small kernel,
 * nothing of their size is copied).  out[0] iteration pairs run, out[1] pairs that started cold on a
 * domain with area boundaries (stand-alone boundary pass + reduction in front: after single iterations, an upload, a new target
 * time), out[2] cells stamped by the LAST pair launch, out[3] cells that carry a stamp of any launch; the exact mode's choice between
 * pairs and single iterations (the same bits; chosen by measurement, hp_engine.hip: tuner_poll): out[4] samples taken, out[5] changes
 * of mind, out[6] 1 if pairs are the current choice, out[7] the last sample's pair time over its two single iterations' time, x 1000;
 * out[8] (exact flavour) stale values taken from a stamp that DIFFERED from the cell's current state -- the cells the flavour without
 * stamps would have got wrong on this run (0: it would have left the same bits); FAST fp64 single domains (the pair kernel's still
 * records; HP_PAIR_SKIP=0 switches them off): out[9] window rows (60 columns each) the LAST pair launch skipped -- found in one
 * still state on their whole stencil by the launch before, neither loaded nor stored -- and out[10] window rows it recorded as
 * still (skipped, or stored as found by a still run; its updated rows x ceil((cols - 2) / 60) in all); out[11] (the same launches'
 * block order; HP_PAIR_ORDER=0 switches it off) tiles the LAST pair launch ran at another position of its band's block stream than
 * tile-row by tile-row order gives them -- 0 where no column group, or every one alike, marched in the launch before, or no table was read. */
int hp_pair_stats(hp_domain_t* d, uint64_t out[12]);
/* The part of out[9] and out[10] that lies in windows next to the edge ring (a window's 60 columns plus its two halo columns either
 * side reach column 0 or cols - 1, or its tile's stencil reaches row 0 or rows - 1): out[0] such window rows the LAST pair launch skipped,
 * out[1] such rows it recorded as still.  There the lake is at rest beside the wall every closed domain has -- dry cells on a high bed
 * that no launch writes -- and the launch has checked, with its own update on its own two timesteps, that this lake stays as it is
 * beside this wall.  HP_PAIR_WALL=0 switches that part off alone (the same bits; A/B runs), HP_PAIR_SKIP=0 with the rest.  Blocks. */
int hp_pair_wall_stats(hp_domain_t* d, uint64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* HIPIMS_MI_H */
