// hp_actors.hpp -- the actors of a domain, host side: what changes the state from outside the flux kernels.  Three kinds: the
// boundaries (uniform, gridded and cell: hp_kernels.hpp), the link groups (hp_links.hpp) and the infiltration (hp_soil.hpp) among them,
// the bed shapes (hp_bed.hpp), and the tracer that rides on the water they move (hp_tracer.hpp).
// Here: their entry points of include/hipims_mi.h, the boundary pass the engine queues in front of an iteration (apply_boundaries)
// and the choice of what the flux kernel carries of it instead (refresh_fusable), and what hp_state_save / hp_state_restore /
// hp_domain_destroy do for their stores (*_save_reserve, *_save, *_restore, *_destroy) and in which order (PARTICIPANTS, the observers included).  Their
// state is declared in hp_domain.hpp (Boundary, BedShapes, LinkStore, SoilStore, TracerStore).  Included once by hp_engine.hip, after hp_observers.hpp: the library
// stays one translation unit.
#pragma once
#include "hp_domain.hpp"
#include "hp_gridded.hpp"
#include <cmath>
#include <cstdlib>

namespace {

static_assert(sizeof(hp_bed_shape_desc_t) == 40 && sizeof(hp_bed_info_t) == 48, "hp_bed_*_t layout");
static_assert(sizeof(hp_link_t) == 56 && sizeof(hp_link_record_t) == 32 && sizeof(LinkDev) == 56, "hp_link_*_t layout");
static_assert(sizeof(hp_soil_class_t) == 32 && sizeof(hp_infiltration_desc_t) == 32, "hp_soil_class_t / hp_infiltration_desc_t layout");
static_assert(sizeof(hp_tracer_desc_t) == 16, "hp_tracer_desc_t layout");
static_assert(sizeof(hp_tracer_set_desc_t) == 24, "hp_tracer_set_desc_t layout");
static_assert(sizeof(hp_tracer_exchange_desc_t) == 48 && sizeof(TracerExchangeParams) == 32, "hp_tracer_exchange_desc_t layout");
static_assert(sizeof(hp_open_segment_t) == 24 && sizeof(hp_open_record_t) == 32 && sizeof(OpenDev) == 24, "hp_open_*_t layout");

// ---- the boundaries ----
// an area boundary as the kernels read it: the stand-alone pass and the fused one are handed the same descriptor
template <typename T> AreaBdy<T> area_bdy(const Boundary& b)
{
	AreaBdy<T> a = AreaBdy<T>{};
	if (b.kind == BDY_UNIFORM) {
		a.kind = 0;
		a.u = UniformBdy<T>{(const T*)b.data, (uint32_t)b.entries, b.definition, (T)b.interval, (T)b.length};
	} else {
		a.kind = 1;
		a.g = GriddedBdy<T>{(const T*)b.data, b.entries, b.grows, b.gcols, b.definition,
		                    (T)b.resolution, (T)b.off_x, (T)b.off_y, (T)b.interval};
	}
	return a;
}

template <typename T> int apply_boundaries(hp_domain* d, void* target)
{
	const Params<T> p = make_params<T>(d);
	const bool truncated = (d->desc.quirks & HP_QUIRK_BDY_TRUNCATED) != 0;
	size_t want = ((size_t)p.cols * p.rows + 255) / 256;
	const dim3 block(256), grid((unsigned)(want < 1024 ? want : 1024));
	// consecutive uniform / gridded boundaries go out as ONE launch (bdy_area); cell boundaries keep their place in
	// the order added (the reference's order is unspecified, quirk Q7; ours is the order of the hp_boundary_add_* calls)
	AreaBdyList<T> list;
	list.count = 0;
	auto flush = [&]() {
		if (list.count == 0) return;
		hipLaunchKernelGGL(bdy_area<T>, grid, block, 0, d->stream, p, (const Scalars<T>*)d->scalars, list, (State4<T>*)target,
		                   (const T*)d->bed, truncated, d->fusable ? (const T*)d->cfl_slot + SLOT_BDY : (const T*)nullptr);
		list.count = 0;
	};
	for (const Boundary& b : d->bdy) {
		if (b.kind == BDY_LINKS) {
			flush();
			hipLaunchKernelGGL(bdy_links<T>, dim3((unsigned)((b.count + 63) / 64)), dim3(64), 0, d->stream, p, (const Scalars<T>*)d->scalars,
			                   (const LinkDev*)b.cells, (unsigned long long)b.count, (State4<T>*)target, (const T*)d->bed, d->links.records + b.entries);
			continue;
		}
		if (b.kind == BDY_OPEN) {
			flush();
			hipLaunchKernelGGL(bdy_open<T>, dim3((unsigned)((b.count + 63) / 64)), dim3(64), 0, d->stream, p, (const Scalars<T>*)d->scalars,
			                   (const OpenDev*)b.cells, (unsigned long long)b.count, (State4<T>*)target, (const T*)d->bed, d->open.records + b.entries);
			continue;
		}
		if (b.kind == BDY_INFILTRATION) {
			flush();
			hipLaunchKernelGGL(bdy_infiltration<T>, soil_grid(p.cols, p.rows), dim3(SOIL_BLOCK), 0, d->stream, p, (const Scalars<T>*)d->scalars,
			                   (const SoilTable*)d->soil.table, (const unsigned char*)d->soil.ids, d->soil.F, (State4<T>*)target, (const T*)d->bed);
			continue;
		}
		if (b.kind == BDY_CELL) {
			flush();
			CellBdy<T> c{(const unsigned long long*)b.cells, b.count, (const T*)b.data, b.entries, b.definition,
			             b.discharge_def, (T)b.interval, (T)b.length};
			hipLaunchKernelGGL(bdy_cell<T>, dim3((unsigned)((b.count + 63) / 64)), dim3(64), 0, d->stream, p,
			                   (const Scalars<T>*)d->scalars, c, (State4<T>*)target, (const T*)d->bed);
			continue;
		}
		if (list.count == AREA_BDY_MAX) flush();
		list.b[list.count++] = area_bdy<T>(b);
	}
	flush();
	HIP_TRY(hipGetLastError());
	return HP_OK;
}

// Which area boundaries the flux kernel carries itself (K1 FUSED, hp_kernels.hpp): Godunov scheme, tuned kernel, nothing but
// uniform / gridded boundaries (a cell boundary or a link group in between has its place in the order added), at most FUSED_BDY_MAX of
// them, and rain grids coarse enough for a tile to meet at most two grid rows and a wavefront two grid columns.  Everything
// else keeps the stand-alone pass.  HP_FUSE_BDY=0 switches the fusion off (A/B runs).
template <typename T> int refresh_fusable_t(hp_domain* d)
{
	d->fusable = false;
	if (!plan_knobs().fuse_bdy || d->desc.scheme != HP_SCHEME_GODUNOV || d->desc.kernel == HP_KERNEL_BASIC) return HP_OK;
	if (d->tracer.on) return HP_OK;                                           // its step stands behind EVERY boundary: none rides in the flux kernel
	if (d->bdy.empty() || d->bdy.size() > (size_t)FUSED_BDY_MAX) return HP_OK;
	AreaBdyList<T> list;
	list.count = 0;
	for (const Boundary& b : d->bdy) {
		if (!is_area(b)) return HP_OK;                                        // a cell boundary or a link group: its place in the order
		if (b.kind == BDY_GRIDDED && b.resolution < 64.0 * d->desc.dx) return HP_OK;
		list.b[list.count++] = area_bdy<T>(b);
	}
	if (!d->fused_list) HIP_TRY(hipMalloc(&d->fused_list, sizeof(AreaBdyList<double>)));
	// the flux launches of a batch still in flight read this list: wait for them before it changes (hp_step_batch returns
	// without waiting, and a blocking copy is not ordered behind a non-blocking stream -- a boundary added right after a
	// batch call used to rain on that batch's remaining iterations; found by the fuzz's boundary-added-mid-run cases)
	HIP_TRY(hipStreamSynchronize(d->stream));
	if (d->stream_halo) HIP_TRY(hipStreamSynchronize(d->stream_halo));
	HIP_TRY(hipMemcpy(d->fused_list, &list, sizeof list, hipMemcpyHostToDevice));
	d->fusable = true;
	return HP_OK;
}

int refresh_fusable(hp_domain* d)
{
	int rc = d->desc.precision == 8 ? refresh_fusable_t<double>(d) : refresh_fusable_t<float>(d);
	// nothing of a next iteration is in any buffer at this point (a batch's last iteration never fuses)
	return rc != HP_OK ? rc : zero_bdy_slot(d);
}

// ---- the moving bed (hp_bed.hpp): the device block of the shapes' lists, and what a checkpoint does for the listed cells ----
BedLists bed_lists(void* block, const BedLayout& l, const size_t n, const unsigned shapes)
{
	char* b = (char*)block;
	BedLists L = {};
	L.cells = (const unsigned long long*)(b + l.cells);
	L.target = (const double*)(b + l.target);
	L.series = (const double*)(b + l.series);
	L.base = b + l.base;
	L.series_off = (const unsigned*)(b + l.series_off);
	L.shape_of = (const unsigned char*)(b + l.shape_of);
	L.count = n;
	L.shapes = shapes;
	return L;
}
void bed_destroy(hp_domain* d) { hipFree(d->beds.block); hipFree(d->beds.info); slot_free(d->beds.saved); }

// What a checkpoint does for the five actors' stores (SaveSlot, hp_domain.hpp): hp_state_save reserves the copy before it touches anything,
// grown with the store or allocated once, and takes it behind the state's copies -- the mark also while the store is off or empty;
// hp_state_restore asks the mark, and what a stale store does stands with its *_restore.  The answer, with the store's `warning` sent if STALE:
Verdict restore_verdict(const SaveSlot& s, const uint64_t epoch, const char* warning)
{
	const Verdict v = s.mark.verdict(epoch);
	if (v == Verdict::STALE) log_line(HP_LOG_WARNING, warning);
	return v;
}
// the bed at the listed cells: gathered into the copy and scattered from it
int bed_save_reserve(hp_domain* d)
{
	BedShapes& B = d->beds;
	return slot_reserve(d->stream, B.saved, B.shapes ? B.lists.count : 0, d->esize, "hp_state_save: cannot allocate the copy of the listed cells' bed: ");
}
// (hp_state_restore brings back neither the bed nor the boundary list, and levels of one bed over another are no state)
int bed_save(hp_domain* d)
{
	BedShapes& B = d->beds;
	B.saved.mark.take(B.epoch);
	if (!B.shapes || !B.lists.count) return HP_OK;
	with_real(d, [&](auto zero) { using T = decltype(zero);
		hipLaunchKernelGGL((bed_gather<T>), dim3(stream_blocks((size_t)B.lists.count)), dim3(256), 0, d->stream, (const T*)d->bed, B.lists.cells, 0ull, B.lists.count, (T*)B.saved.copy);
	});
	HIP_TRY(hipGetLastError());
	return HP_OK;
}
// stale: the bed is left as it is
int bed_restore(hp_domain* d)
{
	BedShapes& B = d->beds;
	const Verdict v = restore_verdict(B.saved, B.epoch, "hp_state_restore: bed shapes were added or cleared after the state was saved: the bed is left as it is");
	if (v != Verdict::BRING_BACK || !B.shapes) return HP_OK;
	d->facts.boundaries_or_bed_changed();
	if (B.lists.count) {
		with_real(d, [&](auto zero) { using T = decltype(zero);
			hipLaunchKernelGGL((bed_scatter<T>), dim3(stream_blocks((size_t)B.lists.count)), dim3(256), 0, d->stream, (T*)d->bed, B.lists.cells, B.lists.count, (const T*)B.saved.copy);
		});
		HIP_TRY(hipGetLastError());
	}
	d->facts.bed_uploaded();
	return HP_OK;
}

// ---- link groups (hp_links.hpp): what a checkpoint and hp_boundary_clear do for the links' records ----
void links_destroy(hp_domain* d) { hipFree(d->links.records); slot_free(d->links.saved); }
inline size_t links_bytes(const LinkStore& L) { return (size_t)L.links * sizeof(hp_link_record_t); }
// hp_boundary_clear: the link groups go with the list, and their records with them
int links_clear(hp_domain* d)
{
	LinkStore& L = d->links;
	if (!L.groups) return HP_OK;
	HIP_TRY(hipMemsetAsync(L.records, 0, links_bytes(L), d->stream));
	L.links = 0;
	L.groups = 0;
	L.taken.clear();
	++L.epoch;
	return HP_OK;
}
// the copy: LINK_MAX records, once the domain has a link
int links_save_reserve(hp_domain* d)
{
	return slot_reserve(d->stream, d->links.saved, d->links.links ? LINK_MAX : 0, sizeof(hp_link_record_t), "hp_state_save: cannot allocate the copy of the links' records: ");
}
int links_save(hp_domain* d) { return slot_take(d->stream, d->links.saved, d->links.records, links_bytes(d->links), d->links.epoch); }
// stale: the records start from zero
int links_restore(hp_domain* d)
{
	LinkStore& L = d->links;
	const Verdict v = restore_verdict(L.saved, L.epoch, "hp_state_restore: link groups were added or cleared after the state was saved: the links' records start from zero");
	if (v == Verdict::STALE && L.links) HIP_TRY(hipMemsetAsync(L.records, 0, links_bytes(L), d->stream));
	return v == Verdict::BRING_BACK ? slot_bring_back(d->stream, L.saved, L.records, links_bytes(L)) : HP_OK;
}

// ---- the infiltration (hp_soil.hpp): what a checkpoint and hp_boundary_clear do for F ----
void soil_destroy(hp_domain* d)
{
	SoilStore& S = d->soil;
	hipFree(S.ids); hipFree(S.F); hipFree(S.table); slot_free(S.saved);
	S.ids = nullptr; S.F = nullptr; S.table = nullptr;
}
// hp_boundary_clear (the stream is idle): the infiltration goes with the list, and F with it
int soil_clear(hp_domain* d)
{
	SoilStore& S = d->soil;
	if (!S.on) return HP_OK;
	soil_destroy(d);
	S.on = false;
	S.classes = 0;
	S.pervious = 0;
	++S.epoch;
	return HP_OK;
}
// the copy: F of every cell, while the domain has an infiltration (hp_boundary_clear frees it with the rest)
inline size_t soil_bytes(const hp_domain* d) { return d->soil.on ? d->cells * sizeof(double) : 0; }
int soil_save_reserve(hp_domain* d)
{
	return slot_reserve(d->stream, d->soil.saved, d->soil.on ? d->cells : 0, sizeof(double), "hp_state_save: cannot allocate the copy of the cumulative infiltration: ");
}
int soil_save(hp_domain* d) { return slot_take(d->stream, d->soil.saved, d->soil.F, soil_bytes(d), d->soil.epoch); }
// stale: F is left as it is
int soil_restore(hp_domain* d)
{
	SoilStore& S = d->soil;
	const Verdict v = restore_verdict(S.saved, S.epoch, "hp_state_restore: the infiltration was added or cleared after the state was saved: the cumulative infiltration is left as it is");
	return v == Verdict::BRING_BACK ? slot_bring_back(d->stream, S.saved, S.F, soil_bytes(d)) : HP_OK;
}

// ---- the open boundary (hp_open.hpp): what a checkpoint and hp_boundary_clear do for its records ----
void open_destroy(hp_domain* d)
{
	OpenStore& O = d->open;
	hipFree(O.records); slot_free(O.saved);
	O.records = nullptr;
	O.room = 0;
}
inline size_t open_bytes(const OpenStore& O) { return (size_t)O.cells * sizeof(hp_open_record_t); }
// hp_boundary_clear (the stream is idle): the segments go with the list, and their records with them
int open_clear(hp_domain* d)
{
	OpenStore& O = d->open;
	if (!O.segments) return HP_OK;
	hipFree(O.records);
	O.records = nullptr;
	O.room = 0;
	O.segments = 0;
	O.cells = 0;
	O.taken.clear();
	++O.epoch;
	return HP_OK;
}
// the copy: a record for every listed cell, grown with the segments
int open_save_reserve(hp_domain* d)
{
	return slot_reserve(d->stream, d->open.saved, d->open.cells, sizeof(hp_open_record_t), "hp_state_save: cannot allocate the copy of the open boundary's records: ");
}
int open_save(hp_domain* d) { return slot_take(d->stream, d->open.saved, d->open.records, open_bytes(d->open), d->open.epoch); }
// stale: the records start from zero
int open_restore(hp_domain* d)
{
	OpenStore& O = d->open;
	const Verdict v = restore_verdict(O.saved, O.epoch, "hp_state_restore: open segments were added or cleared after the state was saved: the open boundary's records start from zero");
	if (v == Verdict::STALE && O.cells) HIP_TRY(hipMemsetAsync(O.records, 0, open_bytes(O), d->stream));
	return v == Verdict::BRING_BACK ? slot_bring_back(d->stream, O.saved, O.records, open_bytes(O)) : HP_OK;
}

// ---- the tracer (hp_tracer.hpp): its launches in front of the flux kernel, and what a checkpoint does for M ----
// One iteration's tracer: the sources onto the current M, then the step from it into the other buffer, which becomes the current one.
// `source`: the state buffer the flux launch of this iteration reads (the boundaries have been applied to it)
template <typename T> int apply_tracer(hp_domain* d, const void* source)
{
	TracerStore& R = d->tracer;
	const Params<T> p = make_params<T>(d);
	if (R.sources && R.lists.count)
		hipLaunchKernelGGL(tracer_sources<T>, dim3(stream_blocks((size_t)R.lists.count)), dim3(256), 0, d->stream, p, (const Scalars<T>*)d->scalars, R.lists, R.M[R.phase]);
	const dim3 block(64, 4), grid((unsigned)((p.cols + 63) / 64), (unsigned)((p.rows + 3) / 4));
	if (R.set && R.exchanging) {                                              // ... and step 7 behind the decay, in place on D
		TracerBedArgs<T, true> X;
		X.D = R.D;
		X.manning = (const T*)d->manning;
		X.exchanging = R.exchanging;
		for (unsigned s = 0; s < HP_TRACER_MAX_SPECIES; ++s) X.of[s] = R.exchange[s];
		hipLaunchKernelGGL((tracer_step_set<T, true>), grid, block, 0, d->stream, p, (const Scalars<T>*)d->scalars, (const T*)d->bed, (const State4<T>*)source,
		                   (const double*)R.M[R.phase], R.M[R.phase ^ 1], R.species, R.rates, X);
	} else if (R.set)                                                         // every species by one launch, the face fluxes formed once
		hipLaunchKernelGGL((tracer_step_set<T, false>), grid, block, 0, d->stream, p, (const Scalars<T>*)d->scalars, (const T*)d->bed, (const State4<T>*)source,
		                   (const double*)R.M[R.phase], R.M[R.phase ^ 1], R.species, R.rates, TracerBedArgs<T, false>{});
	else
		hipLaunchKernelGGL(tracer_step<T>, grid, block, 0, d->stream, p, (const Scalars<T>*)d->scalars, (const T*)d->bed, (const State4<T>*)source,
		                   (const double*)R.M[R.phase], R.M[R.phase ^ 1]);
	HIP_TRY(hipGetLastError());
	R.phase ^= 1;
	++R.iterations;
	return HP_OK;
}
void tracer_destroy(hp_domain* d)
{
	TracerStore& R = d->tracer;
	hipFree(R.M[0]); hipFree(R.M[1]); hipFree(R.D); hipFree(R.block); slot_free(R.saved);
	R.M[0] = R.M[1] = nullptr; R.D = nullptr; R.block = nullptr;
}
// the copy: the current M of every cell and species, then D likewise while the set has one, while the domain has a tracer (hp_tracer_disable
// frees it with the rest); `iterations` goes with it
inline size_t tracer_bytes(const hp_domain* d) { return d->tracer.on ? (size_t)d->tracer.species * d->cells * sizeof(double) : 0; }   // of M; D's are as many
inline size_t tracer_units(const hp_domain* d) { return d->tracer.on ? (d->tracer.D ? 2 : 1) * (size_t)d->tracer.species * d->cells : 0; }
int tracer_save_reserve(hp_domain* d)
{
	return slot_reserve(d->stream, d->tracer.saved, tracer_units(d), sizeof(double), "hp_state_save: cannot allocate the copy of the tracer: ");
}
int tracer_save(hp_domain* d)
{
	TracerStore& R = d->tracer;
	if (R.D) {                                                                // D first, behind M's place: the mark is taken once both copies are queued
		R.saved.mark.drop();
		HIP_TRY(hipMemcpyAsync((char*)R.saved.copy + tracer_bytes(d), R.D, tracer_bytes(d), hipMemcpyDeviceToDevice, d->stream));
	}
	return slot_take(d->stream, R.saved, R.M[R.phase], tracer_bytes(d), R.epoch, R.iterations);
}
// stale: M and D are left as they are.  (The phase names a buffer, nothing more: the saved M goes into the buffer that is current now, and the counter comes back)
int tracer_restore(hp_domain* d)
{
	TracerStore& R = d->tracer;
	const Verdict v = restore_verdict(R.saved, R.epoch, "hp_state_restore: the tracer was enabled or disabled, its species changed or its exchange with the bed began after the state was saved: the tracer is left as it is");
	if (v != Verdict::BRING_BACK || !R.on) return HP_OK;
	int rc = slot_bring_back(d->stream, R.saved, R.M[R.phase], tracer_bytes(d));
	if (rc == HP_OK && R.D) rc = slot_bring_back(d->stream, SaveSlot{(char*)R.saved.copy + tracer_bytes(d), R.saved.mark}, R.D, tracer_bytes(d));
	if (rc == HP_OK) R.iterations = R.saved.mark.count;
	return rc;
}

// ---- who takes part in a checkpoint, in the order hp_state_save (the reserve: before it touches anything; the save), hp_state_restore and
//      hp_domain_destroy go through them: the observers (hp_observers.hpp) before the actors.  The output stage is only freed ----
struct Participant {
	int  (*reserve)(hp_domain*);
	int  (*save)(hp_domain*);
	int  (*restore)(hp_domain*);
	void (*destroy)(hp_domain*);
};
const Participant PARTICIPANTS[] = {
	{nullptr, nullptr, nullptr, out_destroy},
	{peaks_save_reserve, peaks_save, peaks_restore, peaks_destroy},
	{nullptr, probes_save, probes_restore, probes_destroy},
	{nullptr, zones_save, zones_restore, zones_destroy},
	{bed_save_reserve, bed_save, bed_restore, bed_destroy},
	{links_save_reserve, links_save, links_restore, links_destroy},
	{soil_save_reserve, soil_save, soil_restore, soil_destroy},
	{open_save_reserve, open_save, open_restore, open_destroy},
	{tracer_save_reserve, tracer_save, tracer_restore, tracer_destroy},
};
// one phase of a checkpoint (&Participant::reserve, ::save, ::restore): stops at the first participant that fails
int participants_do(hp_domain* d, int (*Participant::*phase)(hp_domain*))
{
	for (const Participant& p : PARTICIPANTS)
		if (p.*phase) { const int rc = (p.*phase)(d); if (rc != HP_OK) return rc; }
	return HP_OK;
}
void participants_destroy(hp_domain* d) { for (const Participant& p : PARTICIPANTS) p.destroy(d); }

} // namespace

// =================================================================================================
extern "C" {

// ---- the moving bed (hp_bed.hpp) ----
int hp_bed_shape_add(hp_domain_t* d, const hp_bed_shape_desc_t* desc)
{
	// argument checks first: none of them touches the device, and those that do not need the domain come before it (validate_bed_shape)
	const std::string who = "hp_bed_shape_add";
	if (!desc) return fail(HP_ERR_INVALID, who + ": desc == NULL");
	if (desc->struct_size != sizeof(hp_bed_shape_desc_t)) return fail(HP_ERR_INVALID, "hp_bed_shape_desc_t size mismatch (ABI)");
	std::vector<uint64_t> listed;
	std::string why;
	if (!validate_bed_shape(desc, d ? &d->beds.host : nullptr, d ? (uint64_t)d->desc.cols : 0, d ? (uint64_t)d->desc.global_rows : 0, listed, why))
		return fail(HP_ERR_INVALID, why);
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, who + " between hp_step_begin and hp_step_end");
	BedShapes& B = d->beds;
	const uint64_t n = desc->cell_count, cols = (uint64_t)d->desc.cols;
	const unsigned m = desc->series_entries;
	// this strip's share: the cells whose row lies in its local array, ghost rows included
	std::vector<uint64_t> cells(B.host.cells);
	std::vector<double> target(B.host.target);
	for (uint64_t k = 0; k < n; ++k) {
		const uint64_t gy = desc->cells[k] / cols, x = desc->cells[k] - gy * cols;
		if (gy < (uint64_t)d->desc.row_offset || gy >= (uint64_t)(d->desc.row_offset + d->desc.rows)) continue;
		cells.push_back((gy - (uint64_t)d->desc.row_offset) * cols + x);
		target.push_back(desc->target[k]);
	}
	const size_t n_old = B.host.cells.size(), n_all = cells.size(), pairs_all = B.host.series.size() / 2 + m;
	const unsigned shapes = B.shapes + 1;
	// the new block first: if it cannot be had, the domain keeps the shapes it has
	const BedLayout l = bed_layout(n_all, pairs_all, shapes, d->esize);
	void* fresh = nullptr;
	if ((rc = alloc_or_fail(&fresh, l.bytes, who + ": cannot allocate the lists: ")) != HP_OK) return rc;
	BedBlock* info = B.info;
	if (!info) {
		if ((rc = alloc_or_fail((void**)&info, sizeof(BedBlock), who + ": cannot allocate the counters: ")) != HP_OK) { hipFree(fresh); return rc; }
	}
	const std::vector<unsigned char> image = bed_image(l, B.host, cells, target, desc->series, m);
	const BedLists L = bed_lists(fresh, l, n_all, shapes);
	hipError_t e = hipMemcpyAsync(fresh, image.data(), l.bytes, hipMemcpyHostToDevice, d->stream);
	if (e == hipSuccess && !B.info) e = hipMemsetAsync(info, 0, sizeof(BedBlock), d->stream);
	// the base of the shapes that are there moves over; the new shape's is the bed as it is now, gathered on the domain's stream
	if (e == hipSuccess && n_old) e = hipMemcpyAsync((char*)fresh + l.base, B.lists.base, n_old * d->esize, hipMemcpyDeviceToDevice, d->stream);
	if (e == hipSuccess && n_all > n_old) {
		with_real(d, [&](auto zero) { using T = decltype(zero);
			hipLaunchKernelGGL((bed_gather<T>), dim3(stream_blocks(n_all - n_old)), dim3(256), 0, d->stream, (const T*)d->bed, L.cells, (unsigned long long)n_old,
			                   (unsigned long long)(n_all - n_old), (T*)((char*)fresh + l.base));
		});
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipStreamSynchronize(d->stream);                 // (queued applies still read the old block; the caller's arrays are free on return)
	if (e != hipSuccess) {
		(void)hipStreamSynchronize(d->stream);
		hipFree(fresh);
		if (!B.info) hipFree(info);
		(void)hipGetLastError();
		return fail(HP_ERR_HIP, who + ": writing the lists: " + hipGetErrorString(e));
	}
	hipFree(B.block);
	B.block = fresh;
	B.info = info;
	B.lists = L;
	B.host.shape_of.resize(n_all, (unsigned char)B.shapes);
	B.shapes = shapes;
	B.host.listed.swap(listed);
	B.host.cells.swap(cells);
	B.host.target.swap(target);
	B.host.series.insert(B.host.series.end(), desc->series, desc->series + 2 * (size_t)m);
	B.host.series_off.push_back((unsigned)pairs_all);
	++B.epoch;
	return HP_OK;
}

int hp_bed_shapes_clear(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	BedShapes& B = d->beds;
	if (!B.shapes) return HP_OK;
	if (d->in_step) return fail(HP_ERR_STATE, "hp_bed_shapes_clear between hp_step_begin and hp_step_end");
	HIP_TRY(hipStreamSynchronize(d->stream));                                 // (queued applies still use the lists)
	bed_destroy(d);
	BedShapes none;
	none.epoch = B.epoch + 1;
	none.saved.mark = B.saved.mark.carried();
	B = none;
	return HP_OK;
}

// By contract exactly the host round trip it replaces -- download state and bed, move the bed and shift the levels, hp_domain_upload
// of the bed, hp_domain_upload of the state --: the kernel patches the buffer hp_domain_download(HP_ARRAY_STATE) reads, and what
// follows it is what the two uploads do, in their order (hp_engine.hip: hp_domain_upload; state_replaced is the state upload's own tail).
int hp_bed_apply(hp_domain_t* d)
{
	int rc = check_domain(d);            // (resolves a pending speculative STRICT batch: an apply never patches a state that is re-run)
	if (rc != HP_OK) return rc;
	BedShapes& B = d->beds;
	if (!B.shapes) return HP_OK;
	if (d->in_step) return fail(HP_ERR_STATE, "hp_bed_apply between hp_step_begin and hp_step_end");
	if (d->facts->ghost_valid != d->ghost_rows)
		return fail(HP_ERR_STATE, "hp_bed_apply: the strip's ghost rows are not all valid (two reaches after an odd number of iterations): apply after an even batch");
	const int cur = d->facts->use_alt;
	const unsigned slot = (unsigned)(B.applies & 1u);
	with_real(d, [&](auto zero) { using T = decltype(zero);
		hipLaunchKernelGGL((bed_apply<T>), dim3(stream_blocks((size_t)B.lists.count)), dim3(256), 0, d->stream, (State4<T>*)d->state[cur], (T*)d->bed,
		                   (const Scalars<T>*)d->scalars, B.lists, B.info, slot);
	});
	HIP_TRY(hipGetLastError());
	++B.applies;
	d->facts.boundaries_or_bed_changed();
	d->facts.buffers_written_outside();
	d->facts.bed_uploaded();
	// both ping-pong buffers hold the patched state, as after hp_domain_upload(HP_ARRAY_STATE)
	HIP_TRY(hipMemcpyAsync(d->state[cur ^ 1], d->state[cur], d->cells * 4 * d->esize, hipMemcpyDeviceToDevice, d->stream));
	return state_replaced(d);
}

int hp_bed_info(hp_domain_t* d, hp_bed_info_t* out)
{
	if (!out) return fail(HP_ERR_INVALID, "hp_bed_info: out == NULL");
	if (out->struct_size != sizeof(hp_bed_info_t)) return fail(HP_ERR_INVALID, "hp_bed_info_t size mismatch (ABI)");
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	const BedShapes& B = d->beds;
	out->shapes = B.shapes;
	out->cells_local = B.lists.count;
	out->applies = B.applies;
	out->changed_last = out->changed_total = 0;
	out->t_last = 0.0;
	if (!B.shapes) return HP_OK;
	BedBlock host;
	HIP_TRY(hipMemcpyAsync(&host, B.info, sizeof host, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));
	if (B.applies) out->changed_last = host.changed[(B.applies - 1) & 1u];
	out->changed_total = host.changed_total;
	out->t_last = host.t_last;
	return HP_OK;
}

// ---- the boundaries ----
int hp_boundary_add_uniform(hp_domain_t* d, int definition, const void* series, uint32_t entries,
                            double interval, double length)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	d->facts.boundaries_or_bed_changed();
	if (!series || entries == 0 || !(interval > 0)) return fail(HP_ERR_INVALID, "bad uniform boundary");
	if (definition != HP_UNIFORM_RAIN_INTENSITY && definition != HP_UNIFORM_LOSS_RATE)
		return fail(HP_ERR_INVALID, "unknown uniform boundary definition");
	Boundary b{};
	b.kind = BDY_UNIFORM; b.definition = definition; b.entries = entries; b.interval = interval; b.length = length;
	if ((rc = upload_or_fail(&b.data, series, (size_t)entries * 2 * d->esize, "hp_boundary_add_uniform: cannot upload the series: ")) != HP_OK) return rc;
	d->bdy.push_back(b);
	return refresh_fusable(d);
}

int hp_boundary_add_gridded(hp_domain_t* d, int definition, const void* grids, uint64_t entries,
                            uint64_t grid_rows, uint64_t grid_cols, double resolution,
                            double offset_x, double offset_y, double interval)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	d->facts.boundaries_or_bed_changed();
	if (!grids || entries == 0 || grid_rows == 0 || grid_cols == 0 || !(resolution > 0) || !(interval > 0))
		return fail(HP_ERR_INVALID, "bad gridded boundary");
	{
		// bdy_Gridded indexes floor((x dx - off) / res) without a range check (CLBoundaries.clc:231-236): a grid that
		// does not cover the interior cells reads outside the buffer.  Rejected here instead, by the kernels' own
		// expression in the domain's precision (hp_gridded.hpp).
		const hp_domain_desc_t& k = d->desc;
		const bool covers = k.precision == 8
			? hp::gridded_covers<double>(k.dx, resolution, offset_x, offset_y, (long)k.cols, (long)k.global_rows, grid_cols, grid_rows)
			: hp::gridded_covers<float>(k.dx, resolution, offset_x, offset_y, (long)k.cols, (long)k.global_rows, grid_cols, grid_rows);
		if (!covers) return fail(HP_ERR_INVALID, "gridded boundary does not cover the domain's interior cells");
	}
	Boundary b{};
	b.kind = BDY_GRIDDED; b.definition = definition; b.entries = entries; b.grows = grid_rows; b.gcols = grid_cols;
	b.resolution = resolution; b.off_x = offset_x; b.off_y = offset_y; b.interval = interval;
	if ((rc = upload_or_fail(&b.data, grids, (size_t)entries * grid_rows * grid_cols * d->esize, "hp_boundary_add_gridded: cannot upload the grids: ")) != HP_OK) return rc;
	d->bdy.push_back(b);
	return refresh_fusable(d);
}

int hp_boundary_add_cell(hp_domain_t* d, int depth_definition, int discharge_definition, const uint64_t* cells,
                         uint64_t count, const void* series, uint64_t entries, double interval, double length)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	d->facts.boundaries_or_bed_changed();
	if (!cells || count == 0 || !series || entries < 2 || !(interval > 0)) return fail(HP_ERR_INVALID, "bad cell boundary");
	if (depth_definition < 0 || depth_definition > 3 || discharge_definition < 0 || discharge_definition > 3)
		return fail(HP_ERR_INVALID, "unknown cell boundary definition");
	const uint64_t global_cells = (uint64_t)d->desc.cols * (uint64_t)d->desc.global_rows;
	bool on_ring = false;
	{
		const uint64_t w = (uint64_t)stencil_reach(d->desc), cols = (uint64_t)d->desc.cols, grows = (uint64_t)d->desc.global_rows;
		for (uint64_t i = 0; i < count; ++i) {
			if (cells[i] >= global_cells) return fail(HP_ERR_INVALID, "cell boundary id outside the grid");
			const uint64_t gy = cells[i] / cols, x = cells[i] - gy * cols;
			on_ring = on_ring || x < w || x + w >= cols || gy < w || gy + w >= grows;
		}
	}
	if (length > (double)(entries - 1) * interval + 1e-9)
		return fail(HP_ERR_INVALID, "cell boundary series shorter than its length (interpolation reads entry n+1)");
	Boundary b{};
	b.kind = BDY_CELL; b.definition = depth_definition; b.discharge_def = discharge_definition; b.count = count;
	b.entries = entries; b.interval = interval; b.length = length;
	if ((rc = upload_or_fail(&b.cells, cells, count * sizeof(uint64_t), "hp_boundary_add_cell: cannot upload the cells: ")) != HP_OK) return rc;
	if ((rc = upload_or_fail(&b.data, series, (size_t)entries * 4 * d->esize, "hp_boundary_add_cell: cannot upload the series: ")) != HP_OK) { hipFree(b.cells); return rc; }
	d->bdy.push_back(b);
	d->bdy_on_ring = d->bdy_on_ring || on_ring;
	return refresh_fusable(d);
}

int hp_boundary_clear(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	d->facts.boundaries_or_bed_changed();
	HIP_TRY(hipStreamSynchronize(d->stream));
	for (auto& b : d->bdy) { hipFree(b.data); hipFree(b.cells); }
	d->bdy.clear();
	d->bdy_on_ring = false;
	if ((rc = links_clear(d)) != HP_OK) return rc;
	if ((rc = soil_clear(d)) != HP_OK) return rc;
	if ((rc = open_clear(d)) != HP_OK) return rc;
	return refresh_fusable(d);
}

// ---- link groups (hp_links.hpp) ----
int hp_boundary_add_links(hp_domain_t* d, const hp_link_t* links, uint64_t count)
{
	// argument checks first: none of them touches the device (hp_links.hpp: validate_links)
	const std::string who = "hp_boundary_add_links";
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (d->tracer.on) return fail(HP_ERR_UNSUPPORTED, who + ": the domain carries a tracer, and the water a link moves would have to carry its share of it");
	LinkStore& L = d->links;
	const uint64_t cols = (uint64_t)d->desc.cols, reach = (uint64_t)stencil_reach(d->desc);
	std::vector<uint64_t> taken;
	std::string why;
	if (!validate_links(links, count, L.links, cols, (uint64_t)d->desc.global_rows, reach, L.taken, taken, why)) return fail(HP_ERR_INVALID, why);
	// this strip's share: both ends of a link, or neither (links_strip_verdict)
	const int64_t lo = d->desc.row_offset, hi = d->desc.row_offset + d->desc.rows;
	const int64_t stale = d->ghost_rows > (int64_t)reach ? d->ghost_rows - (int64_t)reach : 0;      // (two reaches stored: the outer one)
	const int64_t stale_lo = lo > 0 ? stale : 0, stale_hi = hi < d->desc.global_rows ? stale : 0;
	std::vector<LinkDev> dev((size_t)count);
	for (uint64_t k = 0; k < count; ++k) {
		const hp_link_t& l = links[k];
		const int64_t ya = (int64_t)(l.cell_a / cols), yb = (int64_t)(l.cell_b / cols);
		const int verdict = links_strip_verdict(ya, yb, lo, hi, stale_lo, stale_hi);
		if (verdict == LINK_ONE)
			return fail(HP_ERR_UNSUPPORTED, who + ": link " + std::to_string(k) + " (cells " + std::to_string(l.cell_a) + " and " + std::to_string(l.cell_b) +
			            "): this strip stores rows " + std::to_string(lo) + " to " + std::to_string(hi - 1) + " and would hold exactly one of its ends on every iteration");
		LinkDev& o = dev[(size_t)k];
		o.a = verdict == LINK_BOTH ? l.cell_a - (uint64_t)lo * cols : LINK_ABSENT;
		o.b = verdict == LINK_BOTH ? l.cell_b - (uint64_t)lo * cols : LINK_ABSENT;
		o.kind = l.kind; o.one_way = l.one_way; o.level = l.level; o.size = l.size; o.coeff = l.coeff; o.limit = l.limit;
	}
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, who + " between hp_step_begin and hp_step_end");
	if (!L.records) {
		if ((rc = alloc_or_fail((void**)&L.records, (size_t)LINK_MAX * sizeof(hp_link_record_t), who + ": cannot allocate the records: ")) != HP_OK) return rc;
		HIP_TRY(hipMemsetAsync(L.records, 0, (size_t)LINK_MAX * sizeof(hp_link_record_t), d->stream));
	}
	Boundary b{};
	b.kind = BDY_LINKS; b.count = count; b.entries = L.links;
	if ((rc = alloc_or_fail(&b.cells, (size_t)count * sizeof(LinkDev), who + ": cannot allocate the links: ")) != HP_OK) return rc;
	hipError_t e = hipMemcpyAsync(b.cells, dev.data(), (size_t)count * sizeof(LinkDev), hipMemcpyHostToDevice, d->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(d->stream);                 // (`dev` goes with this call)
	if (e != hipSuccess) { hipFree(b.cells); return fail(HP_ERR_HIP, who + ": writing the links: " + hipGetErrorString(e)); }
	d->facts.boundaries_or_bed_changed();
	d->bdy.push_back(b);
	L.links += count;
	L.groups += 1;
	L.taken.swap(taken);
	++L.epoch;
	return refresh_fusable(d);
}

int hp_links_read(hp_domain_t* d, uint64_t first, uint64_t count, hp_link_record_t* out)
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (first > d->links.links || count > d->links.links - first) return fail(HP_ERR_INVALID, "hp_links_read: first + count beyond the domain's links");
	if (count == 0) return HP_OK;
	if (!out) return fail(HP_ERR_INVALID, "hp_links_read: out == NULL");
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, "hp_links_read between hp_step_begin and hp_step_end");
	HIP_TRY(hipMemcpyAsync(out, d->links.records + first, (size_t)count * sizeof(hp_link_record_t), hipMemcpyDeviceToHost, d->stream));
	return HP_OK;
}

int hp_links_info(hp_domain_t* d, uint64_t* links, uint64_t* groups)
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (links) *links = d->links.links;
	if (groups) *groups = d->links.groups;
	return HP_OK;
}

// ---- the infiltration (hp_soil.hpp) ----
int hp_boundary_add_infiltration(hp_domain_t* d, const hp_infiltration_desc_t* desc)
{
	// argument checks first: none of them touches the device (hp_soil.hpp: validate_infiltration)
	const std::string who = "hp_boundary_add_infiltration";
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	uint64_t pervious = 0;
	std::string why;
	if (!validate_infiltration(desc, (uint64_t)d->cells, pervious, why)) return fail(HP_ERR_INVALID, why);
	if (d->tracer.on) return fail(HP_ERR_UNSUPPORTED, who + ": the domain carries a tracer, and the water the soil takes would have to carry its share of it");
	// a strip with two reaches of ghost rows holds the outer one on every second iteration only: F there would drift from its owner's
	if (d->ghost_rows > stencil_reach(d->desc) && (d->desc.row_offset > 0 || d->desc.row_offset + d->desc.rows < d->desc.global_rows))
		return fail(HP_ERR_UNSUPPORTED, who + ": this strip stores two reaches of ghost rows, the outer one valid on every second iteration only: "
		            "the cumulative infiltration there would drift from its owner's (exchange after every iteration instead)");
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, who + " between hp_step_begin and hp_step_end");
	SoilStore& S = d->soil;
	if (S.on) return fail(HP_ERR_STATE, who + ": the domain has an infiltration already (hp_boundary_clear removes it)");
	// everything it needs first: if any of it cannot be had, the domain stays as it is
	SoilTable host;
	soil_table(desc, host);
	unsigned char* ids = nullptr;
	double* F = nullptr;
	SoilTable* table = nullptr;
	if ((rc = alloc_or_fail((void**)&ids, d->cells, who + ": cannot allocate the class ids: ")) != HP_OK) return rc;
	if ((rc = alloc_or_fail((void**)&F, d->cells * sizeof(double), who + ": cannot allocate the cumulative infiltration: ")) != HP_OK) { hipFree(ids); return rc; }
	if ((rc = alloc_or_fail((void**)&table, sizeof(SoilTable), who + ": cannot allocate the class table: ")) != HP_OK) { hipFree(ids); hipFree(F); return rc; }
	hipError_t e = hipMemcpyAsync(ids, desc->soil_of_cell, d->cells, hipMemcpyHostToDevice, d->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(table, &host, sizeof host, hipMemcpyHostToDevice, d->stream);
	if (e == hipSuccess) e = desc->initial ? hipMemcpyAsync(F, desc->initial, d->cells * sizeof(double), hipMemcpyHostToDevice, d->stream)
	                                        : hipMemsetAsync(F, 0, d->cells * sizeof(double), d->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(d->stream);                 // (`host` goes with this call; the caller's arrays are free on return)
	if (e != hipSuccess) {
		(void)hipStreamSynchronize(d->stream);
		hipFree(ids); hipFree(F); hipFree(table);
		(void)hipGetLastError();
		return fail(HP_ERR_HIP, who + ": writing the rasters: " + hipGetErrorString(e));
	}
	Boundary b{};
	b.kind = BDY_INFILTRATION;
	d->facts.boundaries_or_bed_changed();
	d->bdy.push_back(b);
	S.on = true;
	S.ids = ids; S.F = F; S.table = table;
	S.classes = desc->class_count;
	S.pervious = pervious;
	++S.epoch;
	return refresh_fusable(d);
}

int hp_infiltration_read(hp_domain_t* d, double* raster, int64_t row0, int64_t nrows)
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (!raster) return fail(HP_ERR_INVALID, "hp_infiltration_read: raster == NULL");
	int rc = check_rows(d, row0, nrows);
	if (rc != HP_OK) return rc;
	if ((rc = check_domain(d)) != HP_OK) return rc;
	if (!d->soil.on) return fail(HP_ERR_STATE, "hp_infiltration_read: the domain has no infiltration");
	if (d->in_step) return fail(HP_ERR_STATE, "hp_infiltration_read between hp_step_begin and hp_step_end");
	if (nrows == 0) return HP_OK;
	const size_t cols = (size_t)d->desc.cols;
	HIP_TRY(hipMemcpyAsync(raster, d->soil.F + (size_t)row0 * cols, (size_t)nrows * cols * sizeof(double), hipMemcpyDeviceToHost, d->stream));
	return HP_OK;
}

int hp_infiltration_info(hp_domain_t* d, uint32_t* classes, uint64_t* pervious_cells)
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (classes) *classes = d->soil.classes;
	if (pervious_cells) *pervious_cells = d->soil.pervious;
	return HP_OK;
}

// ---- the open boundary (hp_open.hpp) ----
int hp_boundary_add_open(hp_domain_t* d, const hp_open_segment_t* segments, uint32_t count)
{
	// argument checks first: none of them touches the device (hp_open.hpp: validate_open)
	const std::string who = "hp_boundary_add_open";
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	OpenStore& O = d->open;
	const int64_t cols = d->desc.cols, grows = d->desc.global_rows;
	std::vector<uint64_t> taken;
	std::string why;
	if (!validate_open(segments, count, O.segments, cols, grows, O.taken, taken, why)) return fail(HP_ERR_INVALID, why);
	if (d->desc.scheme != HP_SCHEME_GODUNOV)
		return fail(HP_ERR_UNSUPPORTED, who + ": the record of an open cell is the Godunov scheme's face flux; this domain runs another scheme");
	// a strip with two reaches of ghost rows holds the outer one on every second iteration only: the records there would drift from their owners'
	if (d->ghost_rows > stencil_reach(d->desc) && (d->desc.row_offset > 0 || d->desc.row_offset + d->desc.rows < d->desc.global_rows))
		return fail(HP_ERR_UNSUPPORTED, who + ": this strip stores two reaches of ghost rows, the outer one valid on every second iteration only: "
		            "the ring cells there would take stale neighbours (exchange after every iteration instead)");
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, who + " between hp_step_begin and hp_step_end");
	// this strip's share: the ring cells whose row lies in its local array, ghost rows included (open_strip_keeps); every cell has its record slot
	const int64_t lo = d->desc.row_offset, hi = d->desc.row_offset + d->desc.rows;
	std::vector<OpenDev> dev;
	for (uint32_t k = 0; k < count; ++k)
		for (int64_t at = segments[k].first; at <= segments[k].last; ++at) {
			const OpenPlace pl = open_place(segments[k].edge, at, cols, grows);
			OpenDev o;
			o.edge = segments[k].edge; o.pad = 0;
			if (open_strip_keeps(pl.ry, pl.iy, lo, hi)) {
				o.r = (unsigned long long)((pl.ry - lo) * cols + pl.rx);
				o.i = (unsigned long long)((pl.iy - lo) * cols + pl.ix);
			} else {
				o.r = o.i = OPEN_ABSENT;
			}
			dev.push_back(o);
		}
	const uint64_t n = dev.size(), total = O.cells + n;
	// everything it needs first: if any of it cannot be had, the domain stays as it is
	hp_open_record_t* records = nullptr;
	void* cells = nullptr;
	if ((rc = alloc_or_fail((void**)&records, (size_t)total * sizeof(hp_open_record_t), who + ": cannot allocate the records: ")) != HP_OK) return rc;
	if ((rc = alloc_or_fail(&cells, (size_t)n * sizeof(OpenDev), who + ": cannot allocate the cells: ")) != HP_OK) { hipFree(records); return rc; }
	// the records there are move over; the new cells' start from zero.  Queued iterations still write the old block: in stream order
	hipError_t e = hipMemcpyAsync(cells, dev.data(), (size_t)n * sizeof(OpenDev), hipMemcpyHostToDevice, d->stream);
	if (e == hipSuccess && O.cells) e = hipMemcpyAsync(records, O.records, (size_t)O.cells * sizeof(hp_open_record_t), hipMemcpyDeviceToDevice, d->stream);
	if (e == hipSuccess) e = hipMemsetAsync(records + O.cells, 0, (size_t)n * sizeof(hp_open_record_t), d->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(d->stream);                 // (`dev` goes with this call; the old block is free behind it)
	if (e != hipSuccess) {
		(void)hipStreamSynchronize(d->stream);
		hipFree(records); hipFree(cells);
		(void)hipGetLastError();
		return fail(HP_ERR_HIP, who + ": writing the cells: " + hipGetErrorString(e));
	}
	hipFree(O.records);
	O.records = records;
	O.room = total;
	Boundary b{};
	b.kind = BDY_OPEN; b.cells = cells; b.count = n; b.entries = O.cells;
	d->facts.boundaries_or_bed_changed();
	d->bdy.push_back(b);
	d->bdy_on_ring = true;                                                    // ring cells change on every iteration: the ring is priced anew (plan_single)
	O.cells = total;
	O.segments += count;
	O.taken.swap(taken);
	++O.epoch;
	return refresh_fusable(d);
}

int hp_open_read(hp_domain_t* d, uint64_t first, uint64_t count, hp_open_record_t* out)
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (first > d->open.cells || count > d->open.cells - first) return fail(HP_ERR_INVALID, "hp_open_read: first + count beyond the domain's open cells");
	if (count == 0) return HP_OK;
	if (!out) return fail(HP_ERR_INVALID, "hp_open_read: out == NULL");
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, "hp_open_read between hp_step_begin and hp_step_end");
	HIP_TRY(hipMemcpyAsync(out, d->open.records + first, (size_t)count * sizeof(hp_open_record_t), hipMemcpyDeviceToHost, d->stream));
	return HP_OK;
}

int hp_open_info(hp_domain_t* d, uint32_t* segments, uint64_t* cells)
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (segments) *segments = d->open.segments;
	if (cells) *cells = d->open.cells;
	return HP_OK;
}

// ---- the tracer (hp_tracer.hpp) ----
// what hp_tracer_enable and hp_tracer_enable_set share behind their argument checks: the refusals, then `species` planes in each of the
// two buffers (`initial`: that many planes, or NULL for zeros; `decay`: that many rates, or NULL for zeros)
static int tracer_enable_planes(hp_domain_t* d, const std::string& who, const unsigned species, const double* initial, const double* decay, const bool set)
{
	if (d->desc.scheme != HP_SCHEME_GODUNOV)
		return fail(HP_ERR_UNSUPPORTED, who + ": the tracer takes its face fluxes from the Godunov scheme's face solve; this domain runs another scheme");
	if (d->desc.global_rows != d->desc.rows)
		return fail(HP_ERR_UNSUPPORTED, who + ": this domain is a strip of a larger grid: the tracer's ghost rows would need an exchange of their own");
	if (d->links.groups) return fail(HP_ERR_UNSUPPORTED, who + ": the domain has link groups, and the water a link moves would have to carry its share of the tracer");
	if (d->soil.on) return fail(HP_ERR_UNSUPPORTED, who + ": the domain has an infiltration, and the water the soil takes would have to carry its share of the tracer");
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (d->in_step) return fail(HP_ERR_STATE, who + " between hp_step_begin and hp_step_end");
	TracerStore& R = d->tracer;
	if (R.on) return fail(HP_ERR_STATE, who + ": the domain has a tracer already (hp_tracer_disable removes it)");
	// everything it needs first: if any of it cannot be had, the domain stays as it is
	const size_t bytes = (size_t)species * d->cells * sizeof(double);
	double* m0 = nullptr;
	double* m1 = nullptr;
	if ((rc = alloc_or_fail((void**)&m0, bytes, who + ": cannot allocate the tracer: ")) != HP_OK) return rc;
	if ((rc = alloc_or_fail((void**)&m1, bytes, who + ": cannot allocate the tracer's second buffer: ")) != HP_OK) { hipFree(m0); return rc; }
	hipError_t e = initial ? hipMemcpyAsync(m0, initial, bytes, hipMemcpyHostToDevice, d->stream) : hipMemsetAsync(m0, 0, bytes, d->stream);
	if (e == hipSuccess) e = hipMemsetAsync(m1, 0, bytes, d->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(d->stream);                 // (the caller's raster is free on return)
	if (e != hipSuccess) {
		(void)hipStreamSynchronize(d->stream);
		hipFree(m0); hipFree(m1);
		(void)hipGetLastError();
		return fail(HP_ERR_HIP, who + ": writing the raster: " + hipGetErrorString(e));
	}
	d->facts.boundaries_or_bed_changed();
	R.on = true;
	R.set = set;
	R.species = species;
	R.rates = TracerRates{};
	for (unsigned s = 0; decay && s < species; ++s) R.rates.lambda[s] = decay[s];
	R.M[0] = m0; R.M[1] = m1;
	R.phase = 0;
	R.iterations = 0;
	++R.epoch;
	return refresh_fusable(d);
}

int hp_tracer_enable(hp_domain_t* d, const hp_tracer_desc_t* desc)
{
	// argument checks first: none of them touches the device (hp_tracer.hpp: validate_tracer_enable)
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	std::string why;
	if (!validate_tracer_enable(desc, (uint64_t)d->cells, why)) return fail(HP_ERR_INVALID, why);
	return tracer_enable_planes(d, "hp_tracer_enable", 1, desc->initial, nullptr, false);
}

int hp_tracer_enable_set(hp_domain_t* d, const hp_tracer_set_desc_t* desc)
{
	// argument checks first: none of them touches the device (hp_tracer.hpp: validate_tracer_set_enable)
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	std::string why;
	if (!validate_tracer_set_enable(desc, (uint64_t)d->cells, why)) return fail(HP_ERR_INVALID, why);
	return tracer_enable_planes(d, "hp_tracer_enable_set", desc->species, desc->initial, desc->decay, true);
}

int hp_tracer_sources_clear(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	TracerStore& R = d->tracer;
	if (!R.sources) return HP_OK;
	if (d->in_step) return fail(HP_ERR_STATE, "hp_tracer_sources_clear between hp_step_begin and hp_step_end");
	HIP_TRY(hipStreamSynchronize(d->stream));                                 // (queued iterations still use the lists)
	hipFree(R.block);
	R.block = nullptr;
	R.lists = TracerLists{};
	R.sources = 0;
	R.host = TracerHost{};
	return HP_OK;
}

int hp_tracer_disable(hp_domain_t* d)
{
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	TracerStore& R = d->tracer;
	if (!R.on) return HP_OK;
	if (d->in_step) return fail(HP_ERR_STATE, "hp_tracer_disable between hp_step_begin and hp_step_end");
	HIP_TRY(hipStreamSynchronize(d->stream));                                 // (queued iterations still use the buffers)
	tracer_destroy(d);
	d->facts.boundaries_or_bed_changed();
	R.on = false;
	R.set = false;
	R.species = 0;
	R.rates = TracerRates{};
	R.exchanging = 0;
	R.lists = TracerLists{};
	R.sources = 0;
	R.host = TracerHost{};
	R.iterations = 0;
	++R.epoch;
	return refresh_fusable(d);
}

// one source for species `species` (hp_tracer_add_source: species 0)
static int tracer_add_source_to(hp_domain_t* d, const std::string& who, const uint32_t species, const uint64_t* cells, uint64_t count, const double* series, uint32_t entries)
{
	// argument checks first: none of them touches the device (hp_tracer.hpp: validate_tracer_source)
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	TracerStore& R = d->tracer;
	std::vector<uint64_t> listed;
	std::string why;
	if (!validate_tracer_source(cells, count, series, entries, R.host, (uint64_t)d->desc.cols, (uint64_t)d->desc.rows, listed, why, species, std::max(R.species, 1u), who))
		return fail(HP_ERR_INVALID, why);
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!R.on) return fail(HP_ERR_STATE, who + ": the domain has no tracer (hp_tracer_enable)");
	if (d->in_step) return fail(HP_ERR_STATE, who + " between hp_step_begin and hp_step_end");
	TracerHost next = R.host;
	next.cells.insert(next.cells.end(), cells, cells + count);
	next.source_of.resize(next.cells.size(), (unsigned char)R.sources);
	next.species_of.resize(next.cells.size(), (unsigned char)species);
	next.series.insert(next.series.end(), series, series + 2 * (size_t)entries);
	next.series_off.push_back((unsigned)(next.series.size() / 2));
	const unsigned sources = R.sources + 1;
	// the new block first: if it cannot be had, the domain keeps the sources it has
	const TracerLayout l = tracer_layout(next.cells.size(), next.series.size() / 2, sources);
	void* fresh = nullptr;
	if ((rc = alloc_or_fail(&fresh, l.bytes, who + ": cannot allocate the lists: ")) != HP_OK) return rc;
	const std::vector<unsigned char> image = tracer_image(l, next);
	hipError_t e = hipMemcpyAsync(fresh, image.data(), l.bytes, hipMemcpyHostToDevice, d->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(d->stream);                 // (queued iterations still read the old block; `image` goes with this call)
	if (e != hipSuccess) {
		(void)hipStreamSynchronize(d->stream);
		hipFree(fresh);
		(void)hipGetLastError();
		return fail(HP_ERR_HIP, who + ": writing the lists: " + hipGetErrorString(e));
	}
	hipFree(R.block);
	R.block = fresh;
	char* b = (char*)fresh;
	R.lists.cells = (const unsigned long long*)(b + l.cells);
	R.lists.source_of = (const unsigned char*)(b + l.source_of);
	R.lists.species_of = (const unsigned char*)(b + l.species_of);
	R.lists.plane = (unsigned long long)d->cells;
	R.lists.series = (const double*)(b + l.series);
	R.lists.series_off = (const unsigned*)(b + l.series_off);
	R.lists.count = next.cells.size();
	R.lists.sources = sources;
	R.sources = sources;
	next.listed.swap(listed);
	R.host = std::move(next);
	return HP_OK;
}
int hp_tracer_add_source(hp_domain_t* d, const uint64_t* cells, uint64_t count, const double* series, uint32_t entries)
{
	return tracer_add_source_to(d, "hp_tracer_add_source", 0, cells, count, series, entries);
}
int hp_tracer_add_source_to(hp_domain_t* d, uint32_t species, const uint64_t* cells, uint64_t count, const double* series, uint32_t entries)
{
	return tracer_add_source_to(d, "hp_tracer_add_source_to", species, cells, count, series, entries);
}

// the checks hp_tracer_read / hp_tracer_write, their per-species forms and the deposit's share, in the header's order; *plane: species'
// current plane of M, or (`deposit`) its plane of D
static int tracer_plane(hp_domain_t* d, const std::string& who, const uint32_t species, const void* raster, int64_t row0, int64_t nrows, double** plane,
                        const bool deposit = false)
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (!raster) return fail(HP_ERR_INVALID, who + ": raster == NULL");
	const TracerStore& R = d->tracer;
	if (species >= std::max(R.species, 1u))
		return fail(HP_ERR_INVALID, who + ": species " + std::to_string(species) + " of a tracer of " + std::to_string(std::max(R.species, 1u)));
	int rc = check_rows(d, row0, nrows);
	if (rc != HP_OK) return rc;
	if ((rc = check_domain(d)) != HP_OK) return rc;
	if (!R.on) return fail(HP_ERR_STATE, who + ": the domain has no tracer");
	if (d->in_step) return fail(HP_ERR_STATE, who + " between hp_step_begin and hp_step_end");
	if (deposit && !(R.D && R.exchanging)) return fail(HP_ERR_STATE, who + ": no species of the tracer exchanges with a deposit (hp_tracer_set_exchange)");
	*plane = (deposit ? R.D : R.M[R.phase]) + (size_t)species * d->cells + (size_t)row0 * (size_t)d->desc.cols;
	return HP_OK;
}
static int tracer_read_plane(hp_domain_t* d, const std::string& who, uint32_t species, double* raster, int64_t row0, int64_t nrows, const bool deposit = false)
{
	double* plane = nullptr;
	const int rc = tracer_plane(d, who, species, raster, row0, nrows, &plane, deposit);
	if (rc != HP_OK || nrows == 0) return rc;
	HIP_TRY(hipMemcpyAsync(raster, plane, (size_t)nrows * (size_t)d->desc.cols * sizeof(double), hipMemcpyDeviceToHost, d->stream));
	return HP_OK;
}
static int tracer_write_plane(hp_domain_t* d, const std::string& who, uint32_t species, const double* raster, int64_t row0, int64_t nrows, const bool deposit = false)
{
	double* plane = nullptr;
	const int rc = tracer_plane(d, who, species, raster, row0, nrows, &plane, deposit);
	if (rc != HP_OK || nrows == 0) return rc;
	HIP_TRY(hipMemcpyAsync(plane, raster, (size_t)nrows * (size_t)d->desc.cols * sizeof(double), hipMemcpyHostToDevice, d->stream));
	HIP_TRY(hipStreamSynchronize(d->stream));                                 // (the caller's raster is free on return)
	return HP_OK;
}
int hp_tracer_read(hp_domain_t* d, double* raster, int64_t row0, int64_t nrows) { return tracer_read_plane(d, "hp_tracer_read", 0, raster, row0, nrows); }
int hp_tracer_write(hp_domain_t* d, const double* raster, int64_t row0, int64_t nrows) { return tracer_write_plane(d, "hp_tracer_write", 0, raster, row0, nrows); }
int hp_tracer_read_species(hp_domain_t* d, uint32_t species, double* raster, int64_t row0, int64_t nrows)
{
	return tracer_read_plane(d, "hp_tracer_read_species", species, raster, row0, nrows);
}
int hp_tracer_write_species(hp_domain_t* d, uint32_t species, const double* raster, int64_t row0, int64_t nrows)
{
	return tracer_write_plane(d, "hp_tracer_write_species", species, raster, row0, nrows);
}

int hp_tracer_info(hp_domain_t* d, uint64_t* iterations, uint32_t* sources, uint64_t* source_cells)
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	if (iterations) *iterations = d->tracer.on ? d->tracer.iterations : 0;
	if (sources) *sources = d->tracer.sources;
	if (source_cells) *source_cells = (uint64_t)d->tracer.host.cells.size();
	return HP_OK;
}

int hp_tracer_set_info(hp_domain_t* d, uint32_t* species, double* decay)
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	const TracerStore& R = d->tracer;
	if (species) *species = R.on ? R.species : 0;
	for (unsigned s = 0; decay && R.on && s < R.species; ++s) decay[s] = R.rates.lambda[s];
	return HP_OK;
}

// ---- a set's exchange with the bed (hp_tracer.hpp: tracer_exchange) ----
int hp_tracer_set_exchange(hp_domain_t* d, const hp_tracer_exchange_desc_t* desc)
{
	// argument checks first: none of them touches the device (hp_tracer.hpp: validate_tracer_exchange)
	const std::string who = "hp_tracer_set_exchange";
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	TracerStore& R = d->tracer;
	std::string why;
	if (!validate_tracer_exchange(desc, std::max(R.species, 1u), (uint64_t)d->cells, why)) return fail(HP_ERR_INVALID, why);
	int rc = check_domain(d);
	if (rc != HP_OK) return rc;
	if (!R.on) return fail(HP_ERR_STATE, who + ": the domain has no tracer (hp_tracer_enable_set)");
	if (d->in_step) return fail(HP_ERR_STATE, who + " between hp_step_begin and hp_step_end");
	if (!R.set) return fail(HP_ERR_UNSUPPORTED, who + ": the domain's tracer is a single one (hp_tracer_enable), which keeps its own kernel: enable it as a set of one (hp_tracer_enable_set)");
	const size_t plane = d->cells * sizeof(double);
	const bool first = !R.D;
	double* D = R.D;
	// the planes first: if they cannot be had, the domain stays as it is, without exchange
	if (first && (rc = alloc_or_fail((void**)&D, (size_t)R.species * plane, who + ": cannot allocate the deposit: ")) != HP_OK) return rc;
	hipError_t e = first ? hipMemsetAsync(D, 0, (size_t)R.species * plane, d->stream) : hipSuccess;
	if (e == hipSuccess && desc->deposit_initial) e = hipMemcpyAsync(D + (size_t)desc->species * d->cells, desc->deposit_initial, plane, hipMemcpyHostToDevice, d->stream);
	if (e == hipSuccess && (first || desc->deposit_initial)) e = hipStreamSynchronize(d->stream);   // (the caller's raster is free on return)
	if (e != hipSuccess) {
		(void)hipStreamSynchronize(d->stream);
		if (first) hipFree(D);
		(void)hipGetLastError();
		return fail(HP_ERR_HIP, who + ": writing the deposit: " + hipGetErrorString(e));
	}
	if (first) {                                                              // the store changes: an older checkpoint has no D
		R.D = D;
		R.exchanging = 0;
		for (TracerExchangeParams& q : R.exchange) q = TracerExchangeParams{0.0, __builtin_inf(), __builtin_inf(), 0.0};
		++R.epoch;
	}
	R.exchange[desc->species] = TracerExchangeParams{desc->settling, desc->tau_deposit, desc->tau_erode, desc->erodibility};
	const unsigned bit = 1u << desc->species;
	R.exchanging = desc->settling > 0.0 || desc->erodibility > 0.0 ? R.exchanging | bit : R.exchanging & ~bit;
	return HP_OK;
}
int hp_tracer_deposit_read(hp_domain_t* d, uint32_t species, double* raster, int64_t row0, int64_t nrows)
{
	return tracer_read_plane(d, "hp_tracer_deposit_read", species, raster, row0, nrows, true);
}
int hp_tracer_deposit_write(hp_domain_t* d, uint32_t species, const double* raster, int64_t row0, int64_t nrows)
{
	return tracer_write_plane(d, "hp_tracer_deposit_write", species, raster, row0, nrows, true);
}
int hp_tracer_exchange_info(hp_domain_t* d, uint32_t* exchanging_species, hp_tracer_exchange_desc_t out[HP_TRACER_MAX_SPECIES])
{
	if (!d) return fail(HP_ERR_INVALID, "null domain");
	const TracerStore& R = d->tracer;
	const bool has = R.on && R.D;
	if (exchanging_species) *exchanging_species = has ? (uint32_t)__builtin_popcount(R.exchanging) : 0;
	for (unsigned s = 0; out && R.on && s < R.species; ++s) {
		const TracerExchangeParams q = has ? R.exchange[s] : TracerExchangeParams{0.0, __builtin_inf(), __builtin_inf(), 0.0};
		out[s] = hp_tracer_exchange_desc_t{(uint32_t)sizeof(hp_tracer_exchange_desc_t), s, q.settling, q.tau_deposit, q.tau_erode, q.erodibility, nullptr};
	}
	return HP_OK;
}

int hp_boundaries_fused(hp_domain_t* d, int* fused)
{
	if (!d || !fused) return fail(HP_ERR_INVALID, "null argument");
	*fused = d->fusable ? 1 : 0;
	return HP_OK;
}

} // extern "C"
