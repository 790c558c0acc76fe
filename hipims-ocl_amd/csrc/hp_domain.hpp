// hp_domain.hpp -- what the parts of libhipims_mi.so's host side share: the error and log plumbing of the C ABI, struct hp_domain,
// the map of its pinned host block and the helpers more than one part uses (with_real, alloc_or_fail, upload_or_fail, stream_blocks,
// stencil_reach, state_replaced) and the slot a store has in a checkpoint (SaveSlot, slot_*).  Internal to the library's one translation unit: hp_engine.hip includes it, then hp_observers.hpp
// (the code of the four observers whose state is declared here, and of the RecordLog two of them share) and hp_actors.hpp (the code
// of the boundaries, the link groups and the infiltration among them, the moving bed and the tracer: Boundary, LinkStore, SoilStore,
// BedShapes and TracerStore below).
#pragma once
#include "../../include/hipims_mi.h"
#include "hp_facts.hpp"
#include "hp_checkpoint.hpp"
#include "hp_plan.hpp"
#include "hp_kernels.hpp"
#include "hp_peaks.hpp"
#include "hp_probes.hpp"
#include "hp_zones.hpp"
#include "hp_overview.hpp"
#include "hp_sparse.hpp"
#include "hp_bed.hpp"
#include "hp_links.hpp"
#include "hp_soil.hpp"
#include "hp_open.hpp"
#include "hp_tracer.hpp"
#include <rccl/rccl.h>          // types and prototypes only: the library itself is dlopen'ed (hp_comm_load)

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

using namespace hp;

namespace {

thread_local std::string g_last_error;

std::atomic<hp_log_sink_t> g_log_sink{nullptr};
std::atomic<void*>         g_log_user{nullptr};

int fail(int code, const std::string& msg)
{
	g_last_error = msg;
	if (hp_log_sink_t sink = g_log_sink.load(std::memory_order_acquire))
		sink(HP_LOG_MODEL_STOP, g_last_error.c_str(), g_log_user.load(std::memory_order_acquire));
	return code;
}

void log_line(int level, const std::string& msg)
{
	if (hp_log_sink_t sink = g_log_sink.load(std::memory_order_acquire))
		sink(level, msg.c_str(), g_log_user.load(std::memory_order_acquire));
}

#define HIP_TRY(expr)                                                                                  \
	do {                                                                                               \
		hipError_t e_ = (expr);                                                                        \
		if (e_ != hipSuccess)                                                                          \
			return fail(HP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                \
	} while (0)

// Device (or pinned host) memory, or the call fails with `what` + the runtime's reason.  The sticky last error is cleared: the
// launches of later steps ask for it, and this one is dealt with here.
int alloc_or_fail(void** p, const size_t bytes, const std::string& what, const bool pinned = false)
{
	const hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
	if (e == hipSuccess) return HP_OK;
	*p = nullptr;
	(void)hipGetLastError();
	return fail(HP_ERR_HIP, what + hipGetErrorString(e));
}
// ... filled from `host` by a blocking copy (`host` is free on return); a failed copy frees it again
int upload_or_fail(void** dev, const void* host, const size_t bytes, const std::string& what)
{
	const int rc = alloc_or_fail(dev, bytes, what);
	if (rc != HP_OK) return rc;
	const hipError_t e = hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice);
	if (e == hipSuccess) return HP_OK;
	hipFree(*dev);
	*dev = nullptr;
	(void)hipGetLastError();
	return fail(HP_ERR_HIP, what + hipGetErrorString(e));
}

// ---- a store's slot in a checkpoint: hp_state_save's device copy of it and the mark (hp_checkpoint.hpp) ----
struct SaveSlot {
	void*    copy = nullptr;
	SaveMark mark;
};
// hp_state_save, before it touches anything: room for `units` units of `unit_bytes` (`what`: the store's message when it cannot be had).  A
// failure leaves the copy and the mark as they were: the checkpoint before it is untouched
int slot_reserve(hipStream_t stream, SaveSlot& s, const uint64_t units, const size_t unit_bytes, const char* what)
{
	if (!s.mark.needs_room(units)) return HP_OK;
	void* grown = nullptr;
	const int rc = alloc_or_fail(&grown, (size_t)units * unit_bytes, what);
	if (rc != HP_OK) return rc;
	if (s.copy) {
		HIP_TRY(hipStreamSynchronize(stream));                                // (a queued restore may still read the smaller one)
		hipFree(s.copy);
	}
	s.copy = grown;
	s.mark.got_room(units);
	return HP_OK;
}
// ... behind the state's copies: `bytes` of the store as it lies (0 while it is off or empty), and the mark once the copy is queued
int slot_take(hipStream_t stream, SaveSlot& s, const void* store, const size_t bytes, const uint64_t epoch, const uint64_t count = 0)
{
	s.mark.drop();
	if (bytes) HIP_TRY(hipMemcpyAsync(s.copy, store, bytes, hipMemcpyDeviceToDevice, stream));
	s.mark.take(epoch, count);
	return HP_OK;
}
// hp_state_restore, behind the state's copies, for a store whose mark says BRING_BACK
int slot_bring_back(hipStream_t stream, const SaveSlot& s, void* store, const size_t bytes)
{
	if (bytes) HIP_TRY(hipMemcpyAsync(store, s.copy, bytes, hipMemcpyDeviceToDevice, stream));
	return HP_OK;
}
void slot_free(SaveSlot& s) { hipFree(s.copy); s.copy = nullptr; s.mark.lost_room(); }

// a streaming pass over n elements: a few blocks per CU, the rest by grid stride (the result never depends on the shape)
inline unsigned stream_blocks(const size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 2048)); }

// stencil reach of the scheme = ghost rows one iteration consumes, and the width of the never-written edge ring
inline long stencil_reach(const hp_domain_desc_t& desc) { return desc.scheme == HP_SCHEME_MUSCL_HANCOCK ? 2 : 1; }

// ---- the actors' state (their code: hp_actors.hpp) ----
// a boundary, in the order added.  The first two are the AREA boundaries (AreaBdy, hp_kernels.hpp): consecutive ones share a launch
enum BoundaryKind { BDY_UNIFORM, BDY_GRIDDED, BDY_CELL, BDY_LINKS,           // BDY_LINKS: cells is its LinkDev array, entries its first record
                    BDY_INFILTRATION,                                         // BDY_INFILTRATION: everything of it is the domain's SoilStore
                    BDY_OPEN };                                               // BDY_OPEN: cells is its OpenDev array, entries its first record
struct Boundary {
	BoundaryKind kind;
	int      definition;
	int      discharge_def;
	void*    cells;        // device: global cell ids (cell boundaries)
	uint64_t count;
	void*    data;         // device
	uint64_t entries, grows, gcols;
	double   interval, length, resolution, off_x, off_y;
};
inline bool is_area(const Boundary& b) { return b.kind == BDY_UNIFORM || b.kind == BDY_GRIDDED; }

// ---- the observers' state (their code: hp_observers.hpp) ----
// the output stage (hp_output.hpp, hp_overview.hpp, hp_sparse.hpp; hp_domain_derive / hp_domain_overview / hp_domain_sparse / hp_domain_stats):
// allocated on first use
struct OutputStage {
	void*            scratch = nullptr;               // rasters of one block of rows, value after value -- or, of hp_domain_overview, the accumulator
	                                                  // words and elements of one run of block rows, pair after pair; of hp_domain_sparse, the selection words and offsets of the range
	                                                  // and the entries of one run -- (at most OUT_SCRATCH_CAP bytes)
	size_t           scratch_bytes = 0;
	void*            stats = nullptr;                 // STATS_MAX_BLOCKS block partials + the folded result
	void*            stats_host = nullptr;            // pinned: the folded result
};
// the peak tracker (hp_peaks.hpp; hp_peaks_*): nothing of it exists while tracking is off
struct PeakTracker {
	bool             on = false;
	unsigned         mask = 0;                        // HP_PEAK_* bits enabled
	int              count = 0;                       // ... how many: the accumulators lie one after the other in acc, in code order
	double           arrival = 0.0;
	double*          acc = nullptr;                   // count x cells fp64, followed by the PeakBlock
	uint64_t         samples = 0;                     // samples queued since enable / reset (its parity picks the time slot)
	uint64_t         epoch = 0;                       // counts enable / disable: a checkpoint's peaks belong to one epoch
	SaveSlot         saved;                           // hp_state_save's copy of acc (accumulators + block), in bytes; comes back with `samples`
};
// What the probe and the zone recorder share: a log of `capacity` records of `stride` 8-byte words each in device memory, one
// record per sample, and its lifecycle (hp_observers.hpp: log_*).  Nothing of it exists while recording is off.
struct RecordLog {
	bool             on = false;
	void*            input = nullptr;                 // what the recorder's kernel reads besides the state: allocated and freed with the records
	unsigned long long* records = nullptr;            // capacity records of stride 64-bit words (the probes': fp64)
	uint64_t         capacity = 0, stride = 0;
	uint64_t         samples = 0;                     // records queued since enable / reset: the next sample's index
	uint64_t         epoch = 0;                       // counts enable / disable / reset: a checkpoint's count belongs to one epoch
	SaveMark         saved;                           // hp_state_save keeps the sample count only
};
// the probe recorder (hp_probes.hpp; hp_probes_*): log.input holds the lists (`lists` points into it)
struct ProbeRecorder {
	RecordLog        log;
	ProbeLists       lists = {};
};
// the zone recorder (hp_zones.hpp; hp_zones_*): log.input is the id raster of the local array, 2 bytes per cell
struct ZoneRecorder {
	RecordLog        log;
	double           flood_depth = 0.0;
};

// ---- the other actors' state ----
// the moving bed (hp_bed.hpp; hp_bed_*): nothing of it exists while the domain has no shape.  Not an observer: an apply writes the
// bed and the state -- by contract exactly what the two uploads of the host round trip it replaces write
struct BedShapes {
	unsigned         shapes = 0;
	void*            block = nullptr;                 // the lists, one allocation (BedLists points into it)
	BedLists         lists = {};
	BedBlock*        info = nullptr;                  // device: what the applies leave for hp_bed_info
	uint64_t         applies = 0;                     // applies queued since the first shape was added (its parity picks the counter word)
	uint64_t         epoch = 0;                       // counts add / clear: a checkpoint's beds belong to one epoch
	BedHost          host;                            // host copies of the lists: a new shape rewrites the device block as a whole
	SaveSlot         saved;                           // hp_state_save's copy of the bed at the listed cells, in cells
};

// link groups (hp_links.hpp; hp_boundary_add_links): the groups themselves are Boundary entries of kind BDY_LINKS, in the order added; this
// is what they share.  Nothing of it exists while the domain has never had a link
struct LinkStore {
	uint64_t         links = 0;                       // links of all groups
	unsigned         groups = 0;
	hp_link_record_t* records = nullptr;              // device: LINK_MAX records, in the order the links were added
	std::vector<uint64_t> taken;                      // GLOBAL ids of every end of every link, sorted: the repeated-cell check
	uint64_t         epoch = 0;                       // counts add / clear: a checkpoint's records belong to one epoch
	SaveSlot         saved;                           // hp_state_save's copy (LINK_MAX records)
};

// the infiltration (hp_soil.hpp; hp_boundary_add_infiltration): the boundary itself is a Boundary entry of kind BDY_INFILTRATION, at
// most one a domain; this is its state.  Nothing of it exists while the domain has none
struct SoilStore {
	bool             on = false;
	unsigned char*   ids = nullptr;                   // device: the class id of every cell of the local array
	double*          F = nullptr;                     // device: cumulative infiltrated depth, fp64 whatever the domain's precision
	SoilTable*       table = nullptr;                 // device: the classes, indexed by id
	uint32_t         classes = 0;
	uint64_t         pervious = 0;                    // cells of a class other than 0
	uint64_t         epoch = 0;                       // counts add / clear: a checkpoint's F belongs to one epoch
	SaveSlot         saved;                           // hp_state_save's copy of F, in cells
};

// the open boundary (hp_open.hpp; hp_boundary_add_open): its calls are Boundary entries of kind BDY_OPEN, in the order added; this is what
// they share.  Nothing of it exists while the domain has never had an open segment
struct OpenStore {
	uint32_t         segments = 0;
	uint64_t         cells = 0;                       // listed ring cells of all segments (of the GLOBAL grid: a strip has a record slot for each)
	hp_open_record_t* records = nullptr;              // device: `room` records, by segment in the order added, by ascending index inside one
	uint64_t         room = 0;
	std::vector<uint64_t> taken;                      // GLOBAL ids of every listed ring cell, sorted: the repeated-cell check
	uint64_t         epoch = 0;                       // counts add / clear: a checkpoint's records belong to one epoch
	SaveSlot         saved;                           // hp_state_save's copy, in records
};

// the tracer (hp_tracer.hpp; hp_tracer_enable): the solute mass per unit area M, its two buffers and the sources' lists.  Nothing of it
// exists while the domain has none
struct TracerStore {
	bool             on = false;
	bool             set = false;                     // enabled by hp_tracer_enable_set: tracer_step_set moves it (K == 1 included)
	unsigned         species = 0;                     // K: the planes of each buffer, species after species (a single tracer: 1; none: 0)
	TracerRates      rates = {};                      // the species' decay rates (a single tracer: zeros)
	double*          D = nullptr;                     // device: the species' deposits, K planes, from the first hp_tracer_set_exchange on (else NULL)
	unsigned         exchanging = 0;                  // bit s: species s has settling > 0 or erodibility > 0 (tracer_step_set<T, true> while any is set)
	TracerExchangeParams exchange[HP_TRACER_MAX_SPECIES] = {};   // as set (never set: 0, +inf, +inf, 0); meaningful while D exists
	double*          M[2] = {nullptr, nullptr};       // device: M[phase] is the current M, the other one what the next step writes
	int              phase = 0;                       // its own, independent of the state's ping-pong
	uint64_t         iterations = 0;                  // steps since hp_tracer_enable (as restored)
	void*            block = nullptr;                 // device: the sources' lists (TracerLayout), rewritten by every hp_tracer_add_source
	TracerLists      lists = {};
	unsigned         sources = 0;
	TracerHost       host;
	uint64_t         epoch = 0;                       // counts enable / disable / the first hp_tracer_set_exchange: a checkpoint's M and D belong to one epoch
	SaveSlot         saved;                           // hp_state_save's copy of the current M, then D if it exists, in cells; comes back with `iterations`
};

} // namespace

struct hp_domain {
	hp_domain_desc_t desc;
	hipStream_t      stream = nullptr;
	size_t           cells = 0, esize = 0;
	void*            state[2] = {nullptr, nullptr};   // [0] = primary "Cell states", [1] = "Cell states (alternate)"
	void*            bed = nullptr;
	void*            manning = nullptr;
	void*            scalars = nullptr;               // Scalars<T> on the device
	void*            cfl_slot = nullptr;              // CFL_SLOT_BYTES: running max | SLOT_SAVED last used max | SLOT_EDGE ring maxima of [0], [1]
	bool             manning_uniform = false;         // found at upload: one value everywhere -> kernels skip the array
	double           manning_value = 0.0;
	BufferFacts      facts;                           // what the host knows about the state buffers and the slot block between launches, and the
	                                                  // checkpoint's and the speculative batch's copies of it: changed through its events only
	bool             bdy_on_ring = false;             // a cell boundary imposes values on never-written ring cells: re-price every iteration
	int              adv_fresh = 1;                   // does hp_step_end's advance kernel read a new maximum?
	Tiling           tiling;                          // tile heights and row bands of its launches (hp_tiling.hpp: choose_tiling)
	int              sweep_flip = 0;                  // parity of the whole-domain flux launches: every other one visits each band's tiles from
	                                                  // the top down, so that it starts on the rows its predecessor wrote last (sweep_alternates)
	void*            host_scalars = nullptr;          // pinned mirror
	bool             in_step = false;
	std::vector<Boundary> bdy;
	// area boundaries carried by the flux kernel's fused epilogue (K1, FUSED): device copy of their descriptors
	void*            fused_list = nullptr;
	bool             fusable = false;                 // Godunov, tuned kernel, 1..FUSED_BDY_MAX uniform / coarse gridded boundaries, no cell boundary
	int              fuse_next = 0;                   // this iteration is followed by another one of the same batch
	uint64_t         cells_calculated = 0, iterations = 0;
	hipEvent_t       ev_start = nullptr, ev_stop = nullptr;
	// flux-kernel timing samples
	int              timing_stride = 0;
	uint64_t         timing_counter = 0;
	std::vector<std::pair<hipEvent_t, hipEvent_t>> timing_events;   // pool, created by hp_kernel_timing
	size_t           timing_used = 0;
	double           timing_overhead_ms = 0.0;        // an empty event pair's own time (taken off every sample)
	long             own_lo = 0, own_hi = 0;          // rows this rank owns (CFL reduction range)
	// ghost rows of a strip: `ghost_rows` stored per interior side (g or 2g, g = the scheme's stencil reach), of which
	// facts->ghost_valid currently hold their owners' values; an iteration consumes g of them, the exchange refills them all
	long             ghost_rows = 0;
	bool             split_now = false;               // this iteration is followed by an exchange: halo part on its own stream
	// what the ranks told each other at the start of the batch (hp_strip_step_batch): which of them price a new maximum on
	// the iterations that the ping-pong phase alone would not make them price
	bool             strip_any_bdy = false, strip_any_full = false;
	bool             strip_pairs = false;             // the batch's handshake: every rank can run iteration pairs (godunov_march2 over two-reach ghost rows)
	// halo overlap (strip decomposition): the row segments next to the ghost rows run on their own stream so the
	// neighbours' halo transfer can start while the interior segments are still being computed
	bool             halo_overlap = false;
	bool             halo_overlap_set = false;        // the host chose explicitly (hp_set_halo_overlap): comm_init keeps it
	hipStream_t      stream_halo = nullptr;
	hipEvent_t       ev_fork = nullptr, ev_halo = nullptr;
	bool             fork_is_advance = false;         // ev_fork was recorded BY the last advance_time launch
	// strip decomposition driven from C++ (hp_strip_*): one RCCL communicator over the ranks, strip neighbours = rank +- 1
	// device-side checkpoint (hp_state_save / hp_state_restore)
	void*            saved_state = nullptr;
	void*            saved_scalars = nullptr;         // Scalars<T> + the four CFL slots
	bool             saved_valid = false;
	ncclComm_t       comm = nullptr;
	int              comm_rank = 0, comm_world = 1;
	hipEvent_t       ev_xchg = nullptr;               // ghost rows of the iteration in flight have arrived
	// the maximum over all strips through peer-written mailboxes (hp_strip_peer_*; PeerBox in hp_kernels.hpp)
	unsigned long long*  peer_mine = nullptr;         // this rank's mailbox (uncached device memory)
	unsigned long long** peer_table = nullptr;        // device: every rank's mailbox as this device addresses it
	std::vector<void*>   peer_mapped;                 // IPC mappings to close
	int              peer_world = 0, peer_rank = 0;
	bool             peer_agreed = false;             // every rank of the communicator passed the connection test: the strip loop uses them
	uint64_t         peer_rounds = 0;                 // reductions so far (its parity picks the mailbox set; the same on every rank)
	// ghost rows written straight into the neighbours' state buffers (PeerPush): [side: 0 south, 1 north][ping-pong buffer]
	void*            peer_state[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
	long             peer_rows[2] = {0, 0};           // the neighbours' local row counts
	unsigned*        push_arrived = nullptr;          // device counter of the push blocks
	bool             peer_direct = false;             // every rank reached its neighbours' buffers: no transfer library inside an iteration
	bool             push_now = false;                // this iteration's advance kernel carries the ghost rows
	// the flux launch's own tail block instead of a separate advance launch (LaunchTail, hp_kernels.hpp): small launches only
	unsigned long long* tail_words = nullptr;         // one word per flux block (EMPTY between launches)
	bool             fill_now = false;                // this iteration's K1 launch stores the cells the reference leaves untouched as well (dispatch_begin)
	// quirk Q3 across pair launches, exactly (hp_kernels.hpp: PairAux): stamps of the cells whose first-step stale value the next launch needs
	void*            z_state = nullptr;               // stamp records, one per cell: State4<T> + the number of the pair launch that wrote it (allocated with the first pair)
	unsigned long long* haz_words = nullptr;          // two words: [g & 1] == g <=> pair launch g stamped something
	unsigned         pair_gen = 0;                    // number of the last pair launch -- the one that wrote the current state while facts->other_stale holds
	// still records of the FAST fp64 pair kernel (hp_kernels.hpp: StillRec; round 8): two halves of windows x rows records, the last launch's
	// in half still_rec_half, then four counters (hp_pair_stats, hp_pair_wall_stats).  Valid (facts->still_rec_valid) while no writer of either state buffer has run
	// since that launch other than such launches themselves
	void*            still_rec = nullptr;
	size_t           still_rec_slots = 0;             // records per half
	int              still_rec_half = 0;
	bool             still_rec_last = false;          // the last pair launch wrote records (hp_pair_stats)
	// block order of the same launches (hp_order.hpp; round 18): two table halves of bands x tiles-per-band words -- the one the last launch's
	// tail block wrote in half order_half --, then the flags (a word per band and group), then a counter (hp_pair_stats).  order_shape:
	// the (bands, groups, tall, short segments) the buffer was sized for; order_launch: flux_launches as that launch left it -- the next
	// pair launch reads the table only if it is the domain's very next flux launch and of the same shape; order_read: whether the last did
	unsigned*        order_buf = nullptr;
	int              order_shape[4] = {0, 0, 0, 0};
	int              order_half = 0;
	uint64_t         order_launch = 0;
	bool             order_written = false, order_read = false;
	uint64_t         pair_cold_starts = 0;
	// STRICT: pairs or single iterations, by measurement (pair_tuner: the two are the same bits; which is faster depends on how much of
	// the water stands still)
	hipEvent_t       tune_ev[4] = {nullptr, nullptr, nullptr, nullptr};
	int              tune_phase = 0;                  // 0: sample at the next opportunity, 1: a sample is in flight, 2: decided
	bool             tune_prefer_pairs = true;
	uint64_t         tune_next = 0;                   // iteration count from which the next sample is due
	uint64_t         tune_samples = 0, tune_switches = 0;
	float            tune_pair_ms = 0.f, tune_single_ms = 0.f;
	uint64_t         pairs = 0;                       // iteration pairs run by it
	unsigned         single_streak = 0;               // single iterations since the last pair (step_begin_impl: which launches hp_kernel_timing samples)
	uint64_t         flux_launches = 0, flux_launches_tailed = 0;   // whole-domain flux launches of hp_step_batch / hp_strip_step_batch, and how many carried their own tail block
	bool             tail_failed = false;             // a tail block gave up waiting (SLOT_TAIL_ERR seen by the host): the domain is unusable
	bool             strip_first = false;             // hp_strip_step_batch: the batch's first iteration
	bool             tail_allowed = false;            // inside hp_step_batch / hp_strip_step_batch (the host-driven split step has work in between)
	bool             tail_want = false;               // step_begin_impl: this iteration qualifies, if the launch is small enough
	int              tail_fresh = 0;                  // ... and this is what its advance would be told
	bool             tail_done = false;               // launch_march: the launch carried it -- hp_step_end launches nothing
	// speculative STRICT fp64 batches (hp_math.hpp: div_shared; spec_begin / spec_resolve below)
	bool             spec_now = false;                // the flux launches queued now are the shared-reciprocal instantiations
	uint32_t         spec_pending = 0;                // iterations of a speculative batch whose flag word has not been looked at yet
	void*            spec_state = nullptr;            // snapshot in front of the batch: both state buffers ...
	void*            spec_scalars = nullptr;          // ... Scalars<T> + the slot block
	struct { int adv_fresh; uint64_t cells_calculated, iterations; } spec_host;   // ... and what the host counts besides the facts
	uint64_t         spec_batches = 0, spec_replays = 0;
	OutputStage      out;
	PeakTracker      peaks;
	ProbeRecorder    probes;
	ZoneRecorder     zones;
	BedShapes        beds;
	LinkStore        links;
	SoilStore        soil;
	OpenStore        open;
	TracerStore      tracer;
};

namespace {

// The pinned host block (hp_domain::host_scalars): byte offsets of its regions, each up to the next one's
constexpr size_t HOST_PEAKS      = 128;     // the PeakBlock read back by hp_peaks_info
constexpr size_t HOST_HANDSHAKE  = 256;     // the strips' handshakes: 8 elements out, and at + 128 the 8 that came back
constexpr size_t HOST_TAIL_ERR   = 448;     // the sticky word of a tail block that gave up (tail_error_queue)
constexpr size_t HOST_SPEC_FLAG  = 464;     // the flag word of a speculative STRICT batch (spec_resolve)
constexpr size_t HOST_READBACK   = 480;     // the mailboxes' error word and the result of a round (peer_error_check, peer_round_now)
constexpr size_t HOST_RINGS      = 496;     // the verdict of rings_really_differ
constexpr size_t HOST_SCALARS_BYTES = 128, HOST_BLOCK_BYTES = 512;    // Scalars<T> as hp_read_scalars reads them back, at 0; the whole block
static_assert(sizeof(Scalars<double>) <= HOST_SCALARS_BYTES && sizeof(Scalars<float>) <= HOST_SCALARS_BYTES, "Scalars<T> outgrew its region");
static_assert(HOST_SCALARS_BYTES <= HOST_PEAKS && HOST_PEAKS + sizeof(PeakBlock) <= HOST_HANDSHAKE, "pinned block: scalars / peaks");
static_assert(HOST_HANDSHAKE + 128 + 8 * sizeof(double) <= HOST_TAIL_ERR && HOST_TAIL_ERR + sizeof(double) <= HOST_SPEC_FLAG, "pinned block: handshake / tail word");
static_assert(HOST_SPEC_FLAG + 8 <= HOST_READBACK && HOST_READBACK + 16 <= HOST_RINGS && HOST_RINGS + 8 <= HOST_BLOCK_BYTES, "pinned block: flag / read-backs / rings");

int check_domain(hp_domain* d);           // (hp_engine.hip: every entry point that touches the device comes through it)
template <typename T> Params<T> make_params(const hp_domain* d);             // (hp_engine.hip)
const PlanKnobs& plan_knobs();                                               // (hp_engine.hip: the rules' switches, read from the environment once)
template <typename T> int apply_boundaries(hp_domain* d, void* target);      // (hp_actors.hpp: the boundaries, in the order added, onto `target`)
template <typename T> int apply_tracer(hp_domain* d, const void* source);    // (hp_actors.hpp: the tracer's sources and its step on the iteration's source buffer)

// f(T{}) with T = the domain's precision: a launch that differs only in that type is written once
template <typename F> auto with_real(const hp_domain* d, F&& f) { if (d->desc.precision == 8) return f(double{}); return f(float{}); }

// SLOT_BDY (the fused boundaries' contribution to the next maximum) holds nothing of an iteration to come
inline int zero_bdy_slot(hp_domain* d)
{
	HIP_TRY(hipMemsetAsync((char*)d->cfl_slot + (size_t)SLOT_BDY * d->esize, 0, d->esize, d->stream));
	return HP_OK;
}
// Both state buffers have just been queued the same new state (hp_domain_upload(HP_ARRAY_STATE), hp_bed_apply): what goes with it
inline int state_replaced(hp_domain* d)
{
	d->tune_phase = 0;                                                    // (a sample still in flight measured the state that has just been replaced)
	d->facts.full_state_uploaded(d->ghost_rows);                          // (use_alt = 0: CSchemeGodunov.cpp:1075)
	return zero_bdy_slot(d);
}

inline int check_rows(const hp_domain* d, const int64_t row0, const int64_t nrows)
{
	if (row0 < 0 || nrows < 0 || row0 > d->desc.rows || nrows > d->desc.rows - row0) return fail(HP_ERR_INVALID, "row range out of bounds");
	return HP_OK;
}

} // namespace
