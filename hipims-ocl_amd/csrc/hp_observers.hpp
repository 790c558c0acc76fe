// hp_observers.hpp -- the four observers of a domain, host side: the output stage (hp_output.hpp, hp_overview.hpp, hp_sparse.hpp), the peak tracker
// (hp_peaks.hpp), the probe recorder (hp_probes.hpp) and the zone recorder (hp_zones.hpp).  They read the state the solver leaves behind and never change it.  Here:
// their entry points of include/hipims_mi.h, and what hp_state_save / hp_state_restore / hp_domain_destroy do for each of them
// (*_save, *_restore, *_destroy; hp_actors.hpp's PARTICIPANTS lists them in order).  The two recorders share one record log (log_*): their own entry points keep the argument
// checks, what they upload and the launch.  Their state is declared in hp_domain.hpp (OutputStage, PeakTracker, RecordLog, ProbeRecorder, ZoneRecorder).  Included
// once by hp_engine.hip, after hp_domain.hpp: the library stays one translation unit.
#pragma once
#include "hp_domain.hpp"
#include <algorithm>
#include <cstring>

namespace {

static_assert(OUT_VALUES == HP_OUT_COUNT && OUT_FROUDE == HP_OUT_FROUDE && OUT_DEPTH == HP_OUT_DEPTH, "hp_output.hpp and hipims_mi.h disagree");
static_assert(sizeof(hp_domain_stats_t) == 64, "hp_domain_stats_t layout");
static_assert(PEAK_VALUES == HP_PEAK_COUNT && PEAK_SPEED == HP_PEAK_SPEED && PEAK_UNIT_DISCHARGE == HP_PEAK_UNIT_DISCHARGE &&
              PEAK_HAZARD == HP_PEAK_HAZARD && PEAK_ARRIVAL_TIME == HP_PEAK_ARRIVAL_TIME && PEAK_WET_DURATION == HP_PEAK_WET_DURATION,
              "hp_peaks.hpp and hipims_mi.h disagree");
static_assert(sizeof(hp_peaks_desc_t) == 16, "hp_peaks_desc_t layout");
static_assert(sizeof(hp_probes_desc_t) == 64, "hp_probes_desc_t layout");
static_assert(sizeof(hp_zones_desc_t) == 32, "hp_zones_desc_t layout");
static_assert(ZONE_WORDS == HP_ZONE_WORDS, "hp_zones.hpp and hipims_mi.h disagree");
static_assert(AGG_MAX == HP_AGG_MAX && AGG_MIN == HP_AGG_MIN && AGG_COUNT == HP_AGG_COUNT && AGG_KINDS == HP_AGG_KINDS && OVERVIEW_PAIRS == 27, "hp_overview.hpp and hipims_mi.h disagree");

// The value list of hp_domain_derive / hp_peaks_read (`limit` values exist, spelt `limit_name`): none of these checks touches the
// device or needs the domain.  `seen`: the mask of the values listed.
int check_value_list(const std::string& who, const int* values, int count, int limit, const char* limit_name, int element_bytes, void* const* rasters, unsigned& seen)
{
	if (count < 1 || count > limit) return fail(HP_ERR_INVALID, who + ": count outside 1.." + limit_name);
	if (!values || !rasters) return fail(HP_ERR_INVALID, who + ": values / rasters == NULL");
	if (element_bytes != 4 && element_bytes != 8) return fail(HP_ERR_INVALID, who + ": element_bytes must be 4 or 8");
	seen = 0;
	for (int k = 0; k < count; ++k) {
		if (values[k] < 0 || values[k] >= limit) return fail(HP_ERR_INVALID, who + ": unknown value " + std::to_string(values[k]));
		if (seen & (1u << values[k])) return fail(HP_ERR_INVALID, who + ": value " + std::to_string(values[k]) + " listed twice");
		seen |= 1u << values[k];
		if (!rasters[k]) return fail(HP_ERR_INVALID, who + ": rasters[" + std::to_string(k) + "] == NULL");
	}
	return HP_OK;
}

// Cap of the raster scratch.  A request that needs more is worked through in blocks of rows; the kernel of a block runs in
// well under a hundredth of the time its rasters take to cross the host link, so blocks are queued one after the other on the
// domain's stream and nothing would be won by overlapping them.
constexpr size_t OUT_SCRATCH_CAP = (size_t)256 << 20;

// The raster scratch of the output stage, at least `need` bytes.  The new block first: if it cannot be had, the smaller one
// that served so far stays.
int out_scratch_reserve(hp_domain* d, const size_t need, const std::string& who)
{
	if (need <= d->out.scratch_bytes) return HP_OK;
	void* grown = nullptr;
	int rc = alloc_or_fail(&grown, need, who + ": cannot allocate " + std::to_string(need) + " bytes of raster scratch: ");
	if (rc != HP_OK) return rc;
	if (d->out.scratch) {
		hipError_t e2 = hipStreamSynchronize(d->stream);              // (an earlier call's copies may still be reading the old block)
		if (e2 == hipSuccess) e2 = hipFree(d->out.scratch);
		if (e2 != hipSuccess) { hipFree(grown); return fail(HP_ERR_HIP, who + ": releasing the raster scratch: " + hipGetErrorString(e2)); }
	}
	d->out.scratch = grown;
	d->out.scratch_bytes = need;
	return HP_OK;
}

// Rows [row0, row0 + nrows) of `count` rasters of `esize`-byte elements, through the raster scratch to the host: in blocks of
// rows of at most OUT_SCRATCH_CAP bytes.  queue(first, n) queues what fills the scratch for the n cells from cell `first` on,
// value after value (value k at byte k * n * esize); one copy per value follows it.
template <typename Q>
int read_back_blocked(hp_domain* d, const char* who, int count, size_t esize, void* const* rasters, int64_t row0, int64_t nrows, Q&& queue)
{
	const size_t cols = (size_t)d->desc.cols, row_bytes = cols * (size_t)count * esize;      // of all requested rasters together
	const int64_t block_rows = std::max<int64_t>(1, std::min<int64_t>(nrows, (int64_t)(OUT_SCRATCH_CAP / row_bytes)));
	int rc = out_scratch_reserve(d, (size_t)block_rows * row_bytes, who);
	if (rc != HP_OK) return rc;
	for (int64_t r = 0; r < nrows; r += block_rows) {
		const size_t n = (size_t)std::min<int64_t>(block_rows, nrows - r) * cols;
		if ((rc = queue((size_t)(row0 + r) * cols, n)) != HP_OK) return rc;
		for (int k = 0; k < count; ++k)
			HIP_TRY(hipMemcpyAsync((char*)rasters[k] + (size_t)r * cols * esize, (char*)d->out.scratch + (size_t)k * n * esize, n * esize,
			                       hipMemcpyDeviceToHost, d->stream));
	}
	return HP_OK;
}

// ---- the output stage's reduced form: the block grid of a row range (hp_overview_shape; pure arithmetic) ----
constexpr int OVERVIEW_FACTOR_MAX = 4096;
inline void overview_shape(const hp_domain* d, const int factor, const int64_t row0, const int64_t nrows, int64_t* first_block_row, int64_t* block_rows, int64_t* block_cols)
{
	const int64_t lo = d->desc.row_offset + row0;                              // global row of the first one
	*first_block_row = lo / factor;
	*block_rows = nrows == 0 ? 0 : (lo + nrows - 1) / factor - *first_block_row + 1;
	*block_cols = (d->desc.cols + factor - 1) / factor;
}

// ---- the output stage ----
void out_destroy(hp_domain* d) { hipFree(d->out.scratch); hipFree(d->out.stats); if (d->out.stats_host) hipHostFree(d->out.stats_host); }

// ---- the peak tracker ----
inline size_t peaks_bytes(const hp_domain* d) { return (size_t)d->peaks.count * d->cells * sizeof(double) + sizeof(PeakBlock); }
inline PeakBlock* peaks_block(const hp_domain* d) { return (PeakBlock*)(d->peaks.acc + (size_t)d->peaks.count * d->cells); }
// accumulator raster of an enabled value: they lie in code order
inline double* peaks_raster(const hp_domain* d, const int value) { return d->peaks.acc + (size_t)__builtin_popcount(d->peaks.mask & ((1u << value) - 1u)) * d->cells; }

int peaks_reset_queue(hp_domain* d)
{
	const size_t n = (size_t)d->peaks.count * d->cells;
	with_real(d, [&](auto zero) { using T = decltype(zero);
		hipLaunchKernelGGL((peaks_reset<T>), dim3(stream_blocks(n)), dim3(256), 0, d->stream, d->peaks.acc, n, (const Scalars<T>*)d->scalars, peaks_block(d));
	});
	HIP_TRY(hipGetLastError());
	d->peaks.samples = 0;
	return HP_OK;
}

void peaks_destroy(hp_domain* d) { hipFree(d->peaks.acc); slot_free(d->peaks.saved); }

// frees the tracker, the mark of its checkpoint included (the stream is drained first: queued samples and reads still use the accumulators)
int peaks_release(hp_domain* d)
{
	if (!d->peaks.on && !d->peaks.saved.copy) return HP_OK;
	HIP_TRY(hipStreamSynchronize(d->stream));
	peaks_destroy(d);
	const uint64_t epoch = d->peaks.epoch + (d->peaks.on ? 1 : 0);
	d->peaks = PeakTracker{};
	d->peaks.epoch = epoch;
	return HP_OK;
}

// hp_state_save, before it touches anything: the copy of the accumulators has to be there -- if it cannot be had the call fails
// with the checkpoint before it, state and peaks, untouched
int peaks_save_reserve(hp_domain* d)
{
	return slot_reserve(d->stream, d->peaks.saved, d->peaks.on ? peaks_bytes(d) : 0, 1, "hp_state_save: cannot allocate the copy of the peak accumulators: ");
}
// ... and behind the state's copies, while the tracker is on: accumulators and block in one copy.  Off, it keeps no mark
int peaks_save(hp_domain* d)
{
	PeakTracker& P = d->peaks;
	if (P.on) return slot_take(d->stream, P.saved, P.acc, peaks_bytes(d), P.epoch, P.samples);
	P.saved.mark.drop();
	return HP_OK;
}
// hp_state_restore, behind the state's copies, while the tracker is on.  No checkpoint of its own, stale or none at all: the peaks are reset
int peaks_restore(hp_domain* d)
{
	PeakTracker& P = d->peaks;
	if (!P.on) return HP_OK;
	int rc;
	if (P.saved.mark.verdict(P.epoch) == Verdict::BRING_BACK) {
		if ((rc = slot_bring_back(d->stream, P.saved, P.acc, peaks_bytes(d))) == HP_OK) P.samples = P.saved.mark.count;
		return rc;
	}
	if ((rc = peaks_reset_queue(d)) != HP_OK) return rc;                  // (the time block has come back with the state: t_previous is the restored time)
	log_line(HP_LOG_WARNING, "hp_state_restore: the saved state holds no peaks (the tracker was enabled after it was taken): the peaks are reset");
	return HP_OK;
}

// ---- the record log (RecordLog, hp_domain.hpp): everything the probe and the zone recorder do alike.  The calls name the
//      recorder (not its log: their first check may be the null domain) by its public prefix, from which the messages are built
//      when a call fails, and the noun of hp_state_restore's warning ----
struct Recorder { const char* prefix; const char* noun; RecordLog& (*log)(hp_domain*); };
const Recorder PROBES = {"hp_probes", "probe", [](hp_domain* d) -> RecordLog& { return d->probes.log; }};
const Recorder ZONES = {"hp_zones", "zone", [](hp_domain* d) -> RecordLog& { return d->zones.log; }};
constexpr uint64_t PROBES_MAX_GAUGES = 65536, PROBES_MAX_SECTIONS = 1024;
constexpr uint32_t ZONES_MAX = 4096;
constexpr uint64_t LOG_MAX_BYTES = 256ull << 20;                           // of a record buffer

void log_destroy(hp_domain* d, const Recorder& r) { hipFree(r.log(d).input); hipFree(r.log(d).records); }

// frees the recorder (the stream is drained first: queued samples and reads still use its input block and the records).  What
// the recorder keeps next to the log is only read while the log is on.
int log_release(hp_domain* d, const Recorder& r)
{
	RecordLog& g = r.log(d);
	if (!g.on) return HP_OK;
	HIP_TRY(hipStreamSynchronize(d->stream));
	log_destroy(d, r);
	const uint64_t epoch = g.epoch + 1;
	g = RecordLog{};
	g.epoch = epoch;
	return HP_OK;
}

// hp_state_save: the sample count only (the records taken after it are re-recorded by the samples a restore repeats).  Off, it keeps no mark
int log_save(hp_domain* d, const Recorder& r)
{
	RecordLog& g = r.log(d);
	if (g.on) g.saved.take(g.epoch, g.samples); else g.saved.drop();
	return HP_OK;
}
// hp_state_restore, while the recorder is on.  No count of its own, stale or none at all: the count is 0
int log_restore(hp_domain* d, const Recorder& r)
{
	RecordLog& g = r.log(d);
	if (!g.on) return HP_OK;
	const bool mine = g.saved.verdict(g.epoch) == Verdict::BRING_BACK;
	g.samples = mine ? g.saved.count : 0;
	if (!mine) log_line(HP_LOG_WARNING, std::string("hp_state_restore: the saved state holds no ") + r.noun + " sample count (the recorder was enabled or reset after it was taken): the count is 0");
	return HP_OK;
}
// ... of either recorder, by name: what hp_actors.hpp's PARTICIPANTS lists.  (Named functions, not lambdas in the table: hipcc 7 mangled those
// to the very symbols of the accessors in PROBES and ZONES above, _ZN12_GLOBAL__N_1UlP9hp_domainE_8__invokeES1_, and the table called these)
int probes_save(hp_domain* d) { return log_save(d, PROBES); }
int probes_restore(hp_domain* d) { return log_restore(d, PROBES); }
void probes_destroy(hp_domain* d) { log_destroy(d, PROBES); }
int zones_save(hp_domain* d) { return log_save(d, ZONES); }
int zones_restore(hp_domain* d) { return log_restore(d, ZONES); }
void zones_destroy(hp_domain* d) { log_destroy(d, ZONES); }

// <prefix><call> on a recorder that is off, or inside a split step
int log_check_state(hp_domain* d, const Recorder& r, const char* call)
{
	if (!r.log(d).on) return fail(HP_ERR_STATE, std::string(r.prefix) + call + " before " + r.prefix + "_enable");
	if (d->in_step) return fail(HP_ERR_STATE, std::string(r.prefix) + call + " between hp_step_begin and hp_step_end");
	return HP_OK;
}

// <prefix>_enable, first: the descriptor checks every recorder starts with ...
template <typename D> int log_check_desc(const Recorder& r, const D* desc)
{
	if (!desc) return fail(HP_ERR_INVALID, std::string(r.prefix) + "_enable: desc == NULL");
	if (desc->struct_size != sizeof(D)) return fail(HP_ERR_INVALID, std::string(r.prefix) + "_desc_t size mismatch (ABI)");
	if (desc->capacity < 1) return fail(HP_ERR_INVALID, std::string(r.prefix) + "_enable: capacity must be at least 1");
	return HP_OK;
}
// ... behind the recorder's own argument checks, and in front of those that need the domain: the size of the record buffer ...
int log_check_bytes(const Recorder& r, const uint64_t capacity, const uint64_t stride)
{
	if (capacity * stride * 8 > LOG_MAX_BYTES) return fail(HP_ERR_INVALID, std::string(r.prefix) + "_enable: capacity x stride x 8 exceeds 256 MiB");
	return HP_OK;
}
// ... and last: the old recorder goes, the input block (`input_bytes` from `host`; `what` names it) and the record buffer come.
// Returns when the upload has landed: `host` is free again.
int log_open(hp_domain* d, const Recorder& r, const char* what, const void* host, const size_t input_bytes, const uint64_t capacity, const uint64_t stride)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, std::string(r.prefix) + "_enable between hp_step_begin and hp_step_end");
	if ((rc = log_release(d, r)) != HP_OK) return rc;
	RecordLog& g = r.log(d);
	hipError_t e = hipMalloc(&g.input, input_bytes);
	if (e == hipSuccess) e = hipMalloc((void**)&g.records, (size_t)(capacity * stride * 8));
	if (e == hipSuccess) e = hipMemcpyAsync(g.input, host, input_bytes, hipMemcpyHostToDevice, d->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
	if (e != hipSuccess) {
		log_destroy(d, r);
		g.input = nullptr; g.records = nullptr;
		(void)hipGetLastError();
		return fail(HP_ERR_HIP, std::string(r.prefix) + "_enable: cannot allocate " + what + " and the record buffer: " + hipGetErrorString(e));
	}
	g.capacity = capacity;
	g.stride = stride;
	g.samples = 0;
	g.on = true;
	++g.epoch;
	return HP_OK;
}

int log_disable(hp_domain* d, const Recorder& r)
{
	const int rc = check_domain(d);
	return rc != HP_OK ? rc : log_release(d, r);
}

int log_reset(hp_domain* d, const Recorder& r)
{
	int rc = check_domain(d);
	if (rc != HP_OK || (rc = log_check_state(d, r, "_reset")) != HP_OK) return rc;
	r.log(d).samples = 0;                    // (stream order: a read queued before this call has its records before a later sample overwrites them)
	++r.log(d).epoch;
	return HP_OK;
}

// <prefix>_sample, in front of the launch; ++samples follows it
int log_sample_check(hp_domain* d, const Recorder& r)
{
	int rc = check_domain(d);            // (resolves a pending speculative STRICT batch: a sample never sees a state that is re-run)
	if (rc != HP_OK || (rc = log_check_state(d, r, "_sample")) != HP_OK) return rc;
	if (r.log(d).samples >= r.log(d).capacity)
		return fail(HP_ERR_STATE, std::string(r.prefix) + "_sample: the record buffer is full (read the records, then " + r.prefix + "_reset)");
	return HP_OK;
}

// queues the copy of records [first, first + count)
int log_read(hp_domain* d, const Recorder& r, const uint64_t first, const uint64_t count, void* records)
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	int rc = log_check_state(d, r, "_read");
	if (rc != HP_OK) return rc;
	const RecordLog& g = r.log(d);
	if (first > g.samples || count > g.samples - first)
		return fail(HP_ERR_INVALID, std::string(r.prefix) + "_read: first + count beyond the samples taken");
	if (count == 0) return HP_OK;
	if (!records) return fail(HP_ERR_INVALID, std::string(r.prefix) + "_read: records == NULL");
	if ((rc = check_domain(d)) != HP_OK) return rc;
	HIP_TRY(hipMemcpyAsync(records, g.records + first * g.stride, (size_t)(count * g.stride) * 8, hipMemcpyDeviceToHost, d->stream));
	return HP_OK;
}

// host-side counters only
int log_info(hp_domain* d, const Recorder& r, uint64_t* samples, uint64_t* capacity, uint64_t* stride)
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (!r.log(d).on) return fail(HP_ERR_STATE, std::string(r.prefix) + "_info before " + r.prefix + "_enable");
	if (samples) *samples = r.log(d).samples;
	if (capacity) *capacity = r.log(d).capacity;
	if (stride) *stride = r.log(d).stride;
	return HP_OK;
}

} // namespace

// =================================================================================================
extern "C" {

// ---- the output stage on the device (hp_output.hpp) ----
int hp_domain_derive(hp_domain_t* d, const int* values, int count, int element_bytes, void* const* rasters, int64_t row0, int64_t nrows)
{
	// argument checks first: none of them touches the device, and those that do not need the domain come before it
	unsigned seen;
	int rc = check_value_list("hp_domain_derive", values, count, HP_OUT_COUNT, "HP_OUT_COUNT", element_bytes, rasters, seen);
	if (rc != HP_OK) return rc;
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if ((rc = check_rows(d, row0, nrows)) != HP_OK) return rc;
	if (nrows == 0) return HP_OK;
	if ((rc = check_domain(d)) != HP_OK) return rc;
	return read_back_blocked(d, "hp_domain_derive", count, (size_t)element_bytes, rasters, row0, nrows, [&](const size_t first, const size_t n) -> int {
		DeriveTargets t = {};
		for (int k = 0; k < count; ++k) {
			t.raster[values[k]] = (char*)d->out.scratch + (size_t)k * n * (size_t)element_bytes;
			t.mask |= 1u << values[k];
		}
		const dim3 blocks((unsigned)std::min<size_t>((n + 255) / 256, 8192));
		with_real(d, [&](auto zero) { using T = decltype(zero);
			const State4<T>* state = (const State4<T>*)d->state[d->facts->use_alt];      // what hp_domain_download(HP_ARRAY_STATE) reads
			if (element_bytes == 8) hipLaunchKernelGGL((derive_rasters<T, double>), blocks, dim3(256), 0, d->stream, state, (const T*)d->bed, first, n, d->desc.dx, t);
			else hipLaunchKernelGGL((derive_rasters<T, float>), blocks, dim3(256), 0, d->stream, state, (const T*)d->bed, first, n, d->desc.dx, t);
		});
		HIP_TRY(hipGetLastError());
		return HP_OK;
	});
}

int hp_domain_stats(hp_domain_t* d, int64_t row0, int64_t nrows, hp_domain_stats_t* out)
{
	if (!out) return fail(HP_ERR_INVALID, "hp_domain_stats: out == NULL");
	if (out->struct_size != sizeof(hp_domain_stats_t)) return fail(HP_ERR_INVALID, "hp_domain_stats_t size mismatch (ABI)");
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	int rc = check_rows(d, row0, nrows);
	if (rc != HP_OK) return rc;
	out->reserved = 0;
	out->cells = out->cells_wet = 0;
	out->volume = out->max_depth = out->max_speed = 0.0;
	out->max_depth_cell = out->max_speed_cell = UINT64_MAX;
	if (nrows == 0) return HP_OK;
	if ((rc = check_domain(d)) != HP_OK) return rc;
	if (!d->out.stats && (rc = alloc_or_fail(&d->out.stats, (STATS_MAX_BLOCKS + 1) * sizeof(StatsPart), "hp_domain_stats: cannot allocate the block partials: ")) != HP_OK) return rc;
	if (!d->out.stats_host && (rc = alloc_or_fail(&d->out.stats_host, sizeof(StatsPart), "hp_domain_stats: cannot allocate pinned memory: ", true)) != HP_OK) return rc;
	const size_t cols = (size_t)d->desc.cols, n = (size_t)nrows * cols, first = (size_t)row0 * cols;
	// the launch shape is a function of the range alone: the same range is always summed in the same order
	const int blocks = (int)std::min<size_t>((n + 255) / 256, STATS_MAX_BLOCKS);
	StatsPart* partial = (StatsPart*)d->out.stats;
	with_real(d, [&](auto zero) { using T = decltype(zero);
		hipLaunchKernelGGL((domain_stats<T>), dim3(blocks), dim3(256), 0, d->stream, (const State4<T>*)d->state[d->facts->use_alt], (const T*)d->bed, first, n, partial);
	});
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(domain_stats_fold, dim3(1), dim3(256), 0, d->stream, partial, blocks, partial + STATS_MAX_BLOCKS);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(d->out.stats_host, partial + STATS_MAX_BLOCKS, sizeof(StatsPart), hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));
	const StatsPart& s = *(const StatsPart*)d->out.stats_host;
	out->cells = s.cells; out->cells_wet = s.wet;
	out->volume = d->desc.dx * d->desc.dx * s.sum;
	if (s.depth_cell != ~0ull) { out->max_depth = s.max_depth; out->max_depth_cell = s.depth_cell; }
	if (s.speed_cell != ~0ull) { out->max_speed = s.max_speed; out->max_speed_cell = s.speed_cell; }
	return HP_OK;
}

// ---- the output stage's reduced form (hp_overview.hpp) ----
int hp_overview_shape(hp_domain_t* d, int factor, int64_t row0, int64_t nrows, int64_t* first_block_row, int64_t* block_rows, int64_t* block_cols)
{
	if (!first_block_row || !block_rows || !block_cols) return fail(HP_ERR_INVALID, "hp_overview_shape: an output pointer == NULL");
	if (factor < 1 || factor > OVERVIEW_FACTOR_MAX) return fail(HP_ERR_INVALID, "hp_overview_shape: factor outside 1..4096");
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	const int rc = check_rows(d, row0, nrows);
	if (rc != HP_OK) return rc;
	overview_shape(d, factor, row0, nrows, first_block_row, block_rows, block_cols);
	return HP_OK;
}

int hp_domain_overview(hp_domain_t* d, const int* values, const int* aggregates, int count, int factor, int element_bytes, void* const* rasters,
                       int64_t row0, int64_t nrows)
{
	// argument checks first, as in hp_domain_derive: none of them touches the device, and those that do not need the domain come before it
	const std::string who = "hp_domain_overview";
	if (count < 1 || count > OVERVIEW_PAIRS) return fail(HP_ERR_INVALID, who + ": count outside 1..27");
	if (!values || !aggregates || !rasters) return fail(HP_ERR_INVALID, who + ": values / aggregates / rasters == NULL");
	if (element_bytes != 4 && element_bytes != 8) return fail(HP_ERR_INVALID, who + ": element_bytes must be 4 or 8");
	if (factor < 1 || factor > OVERVIEW_FACTOR_MAX) return fail(HP_ERR_INVALID, who + ": factor outside 1..4096");
	OverviewPlan plan;
	std::memset(plan.slot, -1, sizeof plan.slot);
	plan.values = 0;
	unsigned long long kinds = 0;
	for (int k = 0; k < count; ++k) {
		if (values[k] < 0 || values[k] >= HP_OUT_COUNT) return fail(HP_ERR_INVALID, who + ": unknown value " + std::to_string(values[k]));
		if (aggregates[k] < 0 || aggregates[k] >= HP_AGG_KINDS) return fail(HP_ERR_INVALID, who + ": unknown aggregate " + std::to_string(aggregates[k]));
		if (plan.slot[values[k]][aggregates[k]] >= 0)
			return fail(HP_ERR_INVALID, who + ": pair (" + std::to_string(values[k]) + ", " + std::to_string(aggregates[k]) + ") listed twice");
		if (!rasters[k]) return fail(HP_ERR_INVALID, who + ": rasters[" + std::to_string(k) + "] == NULL");
		plan.slot[values[k]][aggregates[k]] = (signed char)k;
		plan.values |= 1u << values[k];
		kinds |= (unsigned long long)aggregates[k] << (2 * k);
	}
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (d->in_step) return fail(HP_ERR_STATE, who + " between hp_step_begin and hp_step_end");
	int rc = check_rows(d, row0, nrows);
	if (rc != HP_OK) return rc;
	if (nrows == 0) return HP_OK;
	if ((rc = check_domain(d)) != HP_OK) return rc;
	int64_t first_block_row, block_rows, block_cols;
	overview_shape(d, factor, row0, nrows, &first_block_row, &block_rows, &block_cols);
	// Scratch of a block row: its accumulator words, pair after pair, and behind them the elements that go to the host.  A request
	// that needs more than the cap is worked through in runs of whole block rows -- cut at multiples of `factor` in GLOBAL rows, so
	// no block is shared between two runs -- queued one after the other like hp_domain_derive's blocks of rows.
	const size_t esize = (size_t)element_bytes, brow_bytes = (size_t)block_cols * (size_t)count * (8 + esize);
	const int64_t run_rows = std::max<int64_t>(1, std::min<int64_t>(block_rows, (int64_t)(OUT_SCRATCH_CAP / brow_bytes)));
	if ((rc = out_scratch_reserve(d, (size_t)run_rows * brow_bytes, who)) != HP_OK) return rc;
	OverviewGeom g = {};
	g.cols = d->desc.cols;
	g.row_offset = d->desc.row_offset;
	g.factor = factor;
	g.block_cols = block_cols;
	g.col_groups = (g.cols + 255) / 256;
	g.resolution = d->desc.dx;
	const long long global_lo = d->desc.row_offset + row0, global_hi = global_lo + nrows;
	for (int64_t b = 0; b < block_rows; b += run_rows) {
		const long long rows_now = std::min<int64_t>(run_rows, block_rows - b);
		g.by0 = first_block_row + b;
		g.g_lo = std::max<long long>(global_lo, g.by0 * factor);
		g.g_hi = std::min<long long>(global_hi, (g.by0 + rows_now) * factor);
		g.blocks = rows_now * block_cols;
		// bands of at most 32 rows, shorter ones while the launch would otherwise leave most of the device idle (the result does
		// not depend on the choice)
		g.band = std::min<long long>(factor, 32);
		const auto items = [&](const long long band) { return rows_now * ((factor + band - 1) / band) * g.col_groups; };
		while (g.band > 4 && items(g.band) < 2048) g.band = (g.band + 1) / 2;
		g.nsub = (factor + g.band - 1) / g.band;
		g.items = items(g.band);
		const size_t words = (size_t)count * (size_t)g.blocks;
		unsigned long long* acc = (unsigned long long*)d->out.scratch;
		char* out = (char*)d->out.scratch + words * 8;
		HIP_TRY(hipMemsetAsync(acc, 0, words * 8, d->stream));                   // "no cell yet" of all three aggregates
		with_real(d, [&](auto zero) { using T = decltype(zero);
			hipLaunchKernelGGL((overview_blocks<T>), dim3((unsigned)std::min<long long>(g.items, 2048)), dim3(256), 0, d->stream,
			                   (const State4<T>*)d->state[d->facts->use_alt], (const T*)d->bed, g, acc, plan);      // what hp_domain_download(HP_ARRAY_STATE) reads
		});
		HIP_TRY(hipGetLastError());
		const dim3 finish((unsigned)std::min<size_t>(((size_t)g.blocks + 255) / 256, 1024), (unsigned)count);
		if (element_bytes == 8) hipLaunchKernelGGL((overview_finish<double>), finish, dim3(256), 0, d->stream, acc, (double*)out, (size_t)g.blocks, kinds);
		else hipLaunchKernelGGL((overview_finish<float>), finish, dim3(256), 0, d->stream, acc, (float*)out, (size_t)g.blocks, kinds);
		HIP_TRY(hipGetLastError());
		for (int k = 0; k < count; ++k)
			HIP_TRY(hipMemcpyAsync((char*)rasters[k] + (size_t)b * (size_t)block_cols * esize, out + (size_t)k * (size_t)g.blocks * esize,
			                       (size_t)g.blocks * esize, hipMemcpyDeviceToHost, d->stream));
	}
	return HP_OK;
}

// ---- the output stage's selected form (hp_sparse.hpp) ----
int hp_domain_sparse(hp_domain_t* d, int select_value, double above, const int* values, int count, int element_bytes, uint64_t capacity,
                     uint64_t* selected, uint64_t* row_ptr, uint32_t* col, void* const* rasters, int64_t row0, int64_t nrows)
{
	// argument checks first, as in hp_domain_derive: none of them touches the device, and those that do not need the domain come before it
	const std::string who = "hp_domain_sparse";
	if (!selected || !row_ptr) return fail(HP_ERR_INVALID, who + ": selected / row_ptr == NULL");
	if (count < 1 || count > HP_OUT_COUNT) return fail(HP_ERR_INVALID, who + ": count outside 1..HP_OUT_COUNT");
	if (!values) return fail(HP_ERR_INVALID, who + ": values == NULL");
	if (element_bytes != 4 && element_bytes != 8) return fail(HP_ERR_INVALID, who + ": element_bytes must be 4 or 8");
	if (select_value < 0 || select_value >= HP_OUT_COUNT) return fail(HP_ERR_INVALID, who + ": unknown select_value " + std::to_string(select_value));
	if (above != above) return fail(HP_ERR_INVALID, who + ": above is a NaN");
	if (capacity > 0 && (!col || !rasters)) return fail(HP_ERR_INVALID, who + ": capacity > 0 with col / rasters == NULL");
	unsigned seen = 0;
	for (int k = 0; k < count; ++k) {
		if (values[k] < 0 || values[k] >= HP_OUT_COUNT) return fail(HP_ERR_INVALID, who + ": unknown value " + std::to_string(values[k]));
		if (seen & (1u << values[k])) return fail(HP_ERR_INVALID, who + ": value " + std::to_string(values[k]) + " listed twice");
		seen |= 1u << values[k];
		if (capacity > 0 && !rasters[k]) return fail(HP_ERR_INVALID, who + ": rasters[" + std::to_string(k) + "] == NULL");
	}
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (d->in_step) return fail(HP_ERR_STATE, who + " between hp_step_begin and hp_step_end");
	int rc = check_rows(d, row0, nrows);
	if (rc != HP_OK) return rc;
	if ((uint64_t)d->desc.cols >= (1ull << 32)) return fail(HP_ERR_INVALID, who + ": cols >= 2^32 do not fit the column type");
	if (nrows == 0) { *selected = 0; row_ptr[0] = 0; return HP_OK; }
	if ((rc = check_domain(d)) != HP_OK) return rc;
	// Scratch: the selection words and the offsets of the range's segments, the device's row_ptr and the scan's tile sums (all 64-bit
	// words), and behind them the entries of one run: value after value, then the columns.
	const uint64_t spr = ((uint64_t)d->desc.cols + 63) / 64, nseg = (uint64_t)nrows * spr;
	const uint64_t tiles = (nseg + SPARSE_SCAN_TILE - 1) / SPARSE_SCAN_TILE;
	const uint64_t fixed = 8 * (2 * nseg + (uint64_t)nrows + 1 + tiles + 1);
	if (nseg > OUT_SCRATCH_CAP / 16 || fixed > OUT_SCRATCH_CAP)
		return fail(HP_ERR_UNSUPPORTED, who + ": the selection words of " + std::to_string(nseg) + " segments exceed the 256 MiB raster scratch");
	const uint64_t esize = (uint64_t)element_bytes, entry_bytes = 4 + (uint64_t)count * esize;
	const uint64_t fit = std::min<uint64_t>(capacity, (OUT_SCRATCH_CAP - fixed) / entry_bytes);      // entries of the largest run
	if (capacity > 0 && fit == 0) return fail(HP_ERR_UNSUPPORTED, who + ": the selection words leave no room for an entry in the 256 MiB raster scratch");
	if ((rc = out_scratch_reserve(d, (size_t)(fixed + fit * entry_bytes), who)) != HP_OK) return rc;
	unsigned long long* const words = (unsigned long long*)d->out.scratch;
	unsigned long long* const offsets = words + nseg;
	unsigned long long* const row_ptr_dev = offsets + nseg;
	unsigned long long* const sums = row_ptr_dev + nrows + 1;
	char* const entries = (char*)(sums + tiles + 1);
	SparseGeom g = {};
	g.cols = d->desc.cols;
	g.row0 = row0;
	g.segs_per_row = (unsigned)spr;
	g.seg_lo = 0;
	g.seg_hi = (unsigned)nseg;
	g.resolution = d->desc.dx;
	const auto wave_blocks = [](const uint64_t segments) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((segments + 3) / 4, 8192))); };
	with_real(d, [&](auto zero) { using T = decltype(zero);
		hipLaunchKernelGGL((sparse_select<T>), wave_blocks(nseg), dim3(256), 0, d->stream,
		                   (const State4<T>*)d->state[d->facts->use_alt], (const T*)d->bed, g, select_value, above, words);      // what hp_domain_download(HP_ARRAY_STATE) reads
	});
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(sparse_scan_sums, dim3((unsigned)tiles), dim3(256), 0, d->stream, words, (unsigned)nseg, sums);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(sparse_scan_top, dim3(1), dim3(256), 0, d->stream, sums, (unsigned)tiles);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(sparse_scan_offsets, dim3((unsigned)tiles), dim3(256), 0, d->stream, words, (unsigned)nseg, sums, (unsigned)tiles, (unsigned)spr, offsets, row_ptr_dev);
	HIP_TRY(hipGetLastError());
	// the one wait of the call: the runs are cut from row_ptr, and the copies are of exactly the selected entries
	HIP_TRY(hipMemcpyAsync(row_ptr, row_ptr_dev, (size_t)(nrows + 1) * 8, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));
	*selected = row_ptr[nrows];
	if (*selected == 0 || *selected > capacity) return HP_OK;
	for (const SparseRun& run : sparse_plan_runs(row_ptr, nrows, entry_bytes, fit * entry_bytes)) {
		SparseTargets t = {};
		for (int k = 0; k < count; ++k) {
			t.raster[values[k]] = entries + (uint64_t)k * run.count * esize;
			t.mask |= 1u << values[k];
		}
		t.col = (unsigned*)(entries + (uint64_t)count * run.count * esize);
		t.first = run.first;
		t.count = run.count;
		g.seg_lo = (unsigned)((uint64_t)run.row_lo * spr);
		g.seg_hi = (unsigned)((uint64_t)run.row_hi * spr);
		with_real(d, [&](auto zero) { using T = decltype(zero);
			const State4<T>* state = (const State4<T>*)d->state[d->facts->use_alt];
			if (element_bytes == 8) hipLaunchKernelGGL((sparse_scatter<T, double>), wave_blocks(g.seg_hi - g.seg_lo), dim3(256), 0, d->stream, state, (const T*)d->bed, g, words, offsets, t);
			else hipLaunchKernelGGL((sparse_scatter<T, float>), wave_blocks(g.seg_hi - g.seg_lo), dim3(256), 0, d->stream, state, (const T*)d->bed, g, words, offsets, t);
		});
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(col + run.first, t.col, (size_t)run.count * 4, hipMemcpyDeviceToHost, d->stream));
		for (int k = 0; k < count; ++k)
			HIP_TRY(hipMemcpyAsync((char*)rasters[k] + run.first * esize, t.raster[values[k]], (size_t)(run.count * esize), hipMemcpyDeviceToHost, d->stream));
	}
	return HP_OK;
}

// ---- the peak tracker (hp_peaks.hpp) ----
int hp_peaks_enable(hp_domain_t* d, const hp_peaks_desc_t* desc)
{
	if (!desc) return fail(HP_ERR_INVALID, "hp_peaks_enable: desc == NULL");
	if (desc->struct_size != sizeof(hp_peaks_desc_t)) return fail(HP_ERR_INVALID, "hp_peaks_desc_t size mismatch (ABI)");
	if (desc->values_mask == 0) return fail(HP_ERR_INVALID, "hp_peaks_enable: values_mask is empty");
	if (desc->values_mask >> HP_PEAK_COUNT) return fail(HP_ERR_INVALID, "hp_peaks_enable: values_mask names an unknown value");
	if (!(desc->arrival_depth >= OUT_WET)) return fail(HP_ERR_INVALID, "hp_peaks_enable: arrival_depth must be at least 1e-8");
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, "hp_peaks_enable between hp_step_begin and hp_step_end");
	if ((rc = peaks_release(d)) != HP_OK) return rc;
	d->peaks.count = __builtin_popcount(desc->values_mask);
	if ((rc = alloc_or_fail((void**)&d->peaks.acc, peaks_bytes(d), "hp_peaks_enable: cannot allocate the accumulators: ")) != HP_OK) { d->peaks.count = 0; return rc; }
	d->peaks.mask = desc->values_mask;
	d->peaks.arrival = desc->arrival_depth;
	d->peaks.on = true;
	++d->peaks.epoch;
	if ((rc = peaks_reset_queue(d)) != HP_OK) { peaks_release(d); return rc; }
	return HP_OK;
}

int hp_peaks_disable(hp_domain_t* d)
{
	const int rc = check_domain(d);
	return rc != HP_OK ? rc : peaks_release(d);
}

int hp_peaks_reset(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!d->peaks.on) return fail(HP_ERR_STATE, "hp_peaks_reset before hp_peaks_enable");
	if (d->in_step) return fail(HP_ERR_STATE, "hp_peaks_reset between hp_step_begin and hp_step_end");
	return peaks_reset_queue(d);
}

int hp_peaks_sample(hp_domain_t* d)
{
	int rc = check_domain(d);            // (resolves a pending speculative STRICT batch: a sample never sees a state that is re-run)
	if (rc != HP_OK) return rc;
	if (!d->peaks.on) return fail(HP_ERR_STATE, "hp_peaks_sample before hp_peaks_enable");
	if (d->in_step) return fail(HP_ERR_STATE, "hp_peaks_sample between hp_step_begin and hp_step_end");
	PeakTargets t = {};
	for (int v = 0; v < HP_PEAK_COUNT; ++v)
		if (d->peaks.mask & (1u << v)) t.acc[v] = peaks_raster(d, v);
	t.mask = d->peaks.mask;
	t.arrival_depth = d->peaks.arrival;
	const unsigned sample = (unsigned)(d->peaks.samples & 1u);          // picks the time slot; `first`: the first sample since enable / reset
	const int first = d->peaks.samples == 0;
	with_real(d, [&](auto zero) { using T = decltype(zero);              // (the buffer hp_domain_download(HP_ARRAY_STATE) reads)
		hipLaunchKernelGGL((track_peaks<T>), dim3(stream_blocks(d->cells)), dim3(256), 0, d->stream, (const State4<T>*)d->state[d->facts->use_alt], (const T*)d->bed,
		                   (const Scalars<T>*)d->scalars, peaks_block(d), sample, first, d->cells, t);
	});
	HIP_TRY(hipGetLastError());
	++d->peaks.samples;
	return HP_OK;
}

int hp_peaks_read(hp_domain_t* d, const int* values, int count, int element_bytes, void* const* rasters, int64_t row0, int64_t nrows)
{
	// argument checks first, as in hp_domain_derive: none of them touches the device
	unsigned seen;
	int rc = check_value_list("hp_peaks_read", values, count, HP_PEAK_COUNT, "HP_PEAK_COUNT", element_bytes, rasters, seen);
	if (rc != HP_OK) return rc;
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (!d->peaks.on) return fail(HP_ERR_STATE, "hp_peaks_read before hp_peaks_enable");
	if (d->in_step) return fail(HP_ERR_STATE, "hp_peaks_read between hp_step_begin and hp_step_end");
	if (seen & ~d->peaks.mask) return fail(HP_ERR_INVALID, "hp_peaks_read: a value that hp_peaks_enable's values_mask does not track");
	if ((rc = check_rows(d, row0, nrows)) != HP_OK) return rc;
	if (nrows == 0) return HP_OK;
	if ((rc = check_domain(d)) != HP_OK) return rc;
	if (element_bytes == 8) {                                             // whole rows are contiguous: the accumulators themselves
		const size_t cols = (size_t)d->desc.cols;
		for (int k = 0; k < count; ++k)
			HIP_TRY(hipMemcpyAsync(rasters[k], peaks_raster(d, values[k]) + (size_t)row0 * cols, (size_t)nrows * cols * sizeof(double),
			                       hipMemcpyDeviceToHost, d->stream));
		return HP_OK;
	}
	return read_back_blocked(d, "hp_peaks_read", count, sizeof(float), rasters, row0, nrows, [&](const size_t first, const size_t n) -> int {
		for (int k = 0; k < count; ++k) {
			hipLaunchKernelGGL(peaks_round, dim3(stream_blocks(n)), dim3(256), 0, d->stream, (const double*)(peaks_raster(d, values[k]) + first),
			                   (float*)d->out.scratch + (size_t)k * n, n);
			HIP_TRY(hipGetLastError());
		}
		return HP_OK;
	});
}

int hp_peaks_info(hp_domain_t* d, uint64_t* samples, double* t_first, double* t_last)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!d->peaks.on) return fail(HP_ERR_STATE, "hp_peaks_info before hp_peaks_enable");
	PeakBlock* host = (PeakBlock*)((char*)d->host_scalars + HOST_PEAKS);
	HIP_TRY(hipMemcpyAsync(host, peaks_block(d), sizeof(PeakBlock), hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));
	if (samples) *samples = d->peaks.samples;
	if (t_first) *t_first = host->t_first;
	if (t_last) *t_last = host->slot[d->peaks.samples & 1u];                 // (sample n - 1 stored its time into slot n & 1)
	return HP_OK;
}

// ---- the probe recorder (hp_probes.hpp) ----
int hp_probes_enable(hp_domain_t* d, const hp_probes_desc_t* desc)
{
	// argument checks first: none of them touches the device
	int rc = log_check_desc(PROBES, desc);
	if (rc != HP_OK) return rc;
	const uint64_t G = desc->gauge_count, S = desc->section_count;
	if (G > PROBES_MAX_GAUGES) return fail(HP_ERR_INVALID, "hp_probes_enable: more than 65536 gauges");
	if (S > PROBES_MAX_SECTIONS) return fail(HP_ERR_INVALID, "hp_probes_enable: more than 1024 sections");
	if (G + S < 1) return fail(HP_ERR_INVALID, "hp_probes_enable: neither a gauge nor a section");
	if (G && !desc->gauge_cells) return fail(HP_ERR_INVALID, "hp_probes_enable: gauge_cells == NULL");
	if (S && (!desc->section_offsets || !desc->section_cells || !desc->section_wx || !desc->section_wy))
		return fail(HP_ERR_INVALID, "hp_probes_enable: a section array == NULL");
	const uint64_t stride = 1 + PROBE_GAUGE_WORDS * G + S;
	if ((rc = log_check_bytes(PROBES, desc->capacity, stride)) != HP_OK) return rc;
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	const uint64_t cells = d->cells;
	for (uint64_t g = 0; g < G; ++g)
		if (desc->gauge_cells[g] >= cells) return fail(HP_ERR_INVALID, "hp_probes_enable: gauge " + std::to_string(g) + ": cell id outside the local array");
	uint64_t M = 0;
	if (S) {
		if (desc->section_offsets[0] != 0) return fail(HP_ERR_INVALID, "hp_probes_enable: section_offsets[0] must be 0");
		for (uint64_t s = 0; s < S; ++s) {
			const uint64_t lo = desc->section_offsets[s], hi = desc->section_offsets[s + 1];
			if (hi < lo || hi - lo < 2) return fail(HP_ERR_INVALID, "hp_probes_enable: section " + std::to_string(s) + " is shorter than 2 entries");
			if (hi > (1ull << 32)) return fail(HP_ERR_INVALID, "hp_probes_enable: section " + std::to_string(s) + ": offsets out of range");
		}
		M = desc->section_offsets[S];
		for (uint64_t e = 0; e < M; ++e) {
			if (desc->section_cells[e] >= cells) return fail(HP_ERR_INVALID, "hp_probes_enable: section entry " + std::to_string(e) + ": cell id outside the local array");
			if (desc->section_wx[e] < -1 || desc->section_wx[e] > 1 || desc->section_wy[e] < -1 || desc->section_wy[e] > 1)
				return fail(HP_ERR_INVALID, "hp_probes_enable: section entry " + std::to_string(e) + ": weight outside {-1, 0, 1}");
		}
	}
	// one block for the lists: [gauge cells | section offsets | section cells | wx | wy], the 8-byte arrays first
	const size_t words = (size_t)(G + (S ? S + 1 : 0) + M);
	const size_t list_bytes = words * 8 + 2 * (size_t)M;
	std::vector<unsigned char> host(list_bytes);
	uint64_t* w = (uint64_t*)host.data();
	if (G) std::memcpy(w, desc->gauge_cells, G * 8);
	if (S) {
		std::memcpy(w + G, desc->section_offsets, (S + 1) * 8);
		std::memcpy(w + G + S + 1, desc->section_cells, M * 8);
		std::memcpy(host.data() + words * 8, desc->section_wx, M);
		std::memcpy(host.data() + words * 8 + M, desc->section_wy, M);
	}
	if ((rc = log_open(d, PROBES, "the lists", host.data(), list_bytes, desc->capacity, stride)) != HP_OK) return rc;
	const unsigned long long* dw = (const unsigned long long*)d->probes.log.input;
	ProbeLists& p = d->probes.lists;
	p.gauge_cells = dw;
	p.section_offsets = dw + G;
	p.section_cells = dw + G + (S ? S + 1 : 0);
	p.section_wx = (const signed char*)d->probes.log.input + words * 8;
	p.section_wy = p.section_wx + M;
	p.gauges = G;
	p.gauge_blocks = (unsigned)((G + 255) / 256);
	p.sections = (unsigned)S;
	return HP_OK;
}

int hp_probes_disable(hp_domain_t* d) { return log_disable(d, PROBES); }
int hp_probes_reset(hp_domain_t* d) { return log_reset(d, PROBES); }

int hp_probes_sample(hp_domain_t* d)
{
	const int rc = log_sample_check(d, PROBES);
	if (rc != HP_OK) return rc;
	RecordLog& g = d->probes.log;
	const ProbeLists& p = d->probes.lists;
	const unsigned blocks = p.gauge_blocks + p.sections;
	// the buffer hp_domain_download(HP_ARRAY_STATE) reads
	with_real(d, [&](auto zero) {
		using T = decltype(zero);
		hipLaunchKernelGGL((record_probes<T>), dim3(blocks), dim3(256), 0, d->stream, (const State4<T>*)d->state[d->facts->use_alt], (const T*)d->bed,
		                   (const Scalars<T>*)d->scalars, p, (double*)g.records, (unsigned long long)g.samples, (unsigned long long)g.stride, d->desc.dx);
	});
	HIP_TRY(hipGetLastError());
	++g.samples;
	return HP_OK;
}

int hp_probes_read(hp_domain_t* d, uint64_t first, uint64_t count, double* records) { return log_read(d, PROBES, first, count, records); }
int hp_probes_info(hp_domain_t* d, uint64_t* samples, uint64_t* capacity, uint64_t* stride) { return log_info(d, PROBES, samples, capacity, stride); }

// ---- the zone recorder (hp_zones.hpp) ----
int hp_zones_enable(hp_domain_t* d, const hp_zones_desc_t* desc)
{
	// argument checks first: none of them touches the device
	int rc = log_check_desc(ZONES, desc);
	if (rc != HP_OK) return rc;
	if (desc->zone_count < 1 || desc->zone_count > ZONES_MAX) return fail(HP_ERR_INVALID, "hp_zones_enable: zone_count outside 1..4096");
	if (!desc->zone_of_cell) return fail(HP_ERR_INVALID, "hp_zones_enable: zone_of_cell == NULL");
	if (!(desc->flood_depth >= OUT_WET)) return fail(HP_ERR_INVALID, "hp_zones_enable: flood_depth must be at least 1e-8");
	const uint64_t stride = 1 + (uint64_t)ZONE_WORDS * desc->zone_count;
	if ((rc = log_check_bytes(ZONES, desc->capacity, stride)) != HP_OK) return rc;
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	const uint64_t cells = d->cells;
	for (uint64_t k = 0; k < cells; ++k)
		if (desc->zone_of_cell[k] > desc->zone_count)
			return fail(HP_ERR_INVALID, "hp_zones_enable: cell " + std::to_string(k) + ": zone id " + std::to_string(desc->zone_of_cell[k]) + " above zone_count");
	if ((rc = log_open(d, ZONES, "the id raster", desc->zone_of_cell, (size_t)cells * sizeof(uint16_t), desc->capacity, stride)) != HP_OK) return rc;
	d->zones.flood_depth = desc->flood_depth;
	return HP_OK;
}

int hp_zones_disable(hp_domain_t* d) { return log_disable(d, ZONES); }
int hp_zones_reset(hp_domain_t* d) { return log_reset(d, ZONES); }

int hp_zones_sample(hp_domain_t* d)
{
	const int rc = log_sample_check(d, ZONES);
	if (rc != HP_OK) return rc;
	RecordLog& g = d->zones.log;
	unsigned long long* rec = g.records + g.samples * g.stride;
	// one fill (the sums start from 0, the maxima from the bit pattern of +0.0), one launch.  The waves split the cells into
	// contiguous runs of a multiple of 64; the record does not depend on the shape.
	HIP_TRY(hipMemsetAsync(rec, 0, (size_t)g.stride * sizeof(uint64_t), d->stream));
	const size_t n = d->cells;
	const unsigned blocks = stream_blocks(n);
	const size_t waves = (size_t)blocks * (256 / 64);
	const size_t per_wave = ((n + waves - 1) / waves + 63) / 64 * 64;
	with_real(d, [&](auto zero) { using T = decltype(zero);              // (the buffer hp_domain_download(HP_ARRAY_STATE) reads)
		hipLaunchKernelGGL((record_zones<T>), dim3(blocks), dim3(256), 0, d->stream, (const State4<T>*)d->state[d->facts->use_alt], (const T*)d->bed,
		                   (const unsigned short*)g.input, (const Scalars<T>*)d->scalars, rec, n, per_wave, d->zones.flood_depth);
	});
	HIP_TRY(hipGetLastError());
	++g.samples;
	return HP_OK;
}

int hp_zones_read(hp_domain_t* d, uint64_t first, uint64_t count, uint64_t* records) { return log_read(d, ZONES, first, count, records); }
int hp_zones_info(hp_domain_t* d, uint64_t* samples, uint64_t* capacity, uint64_t* stride) { return log_info(d, ZONES, samples, capacity, stride); }
} // extern "C"
