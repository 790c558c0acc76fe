// hp_gridded.hpp -- the gridded boundary's lookup, host side: does a rain grid cover the domain's interior cells?  bdy_Gridded indexes
//     col = floor(((T)x * dx - off_x) / resolution),   row = floor(((T)gy * dx - off_y) / resolution)
// without a range check (Boundaries/CLBoundaries.clc:231-236), T being the domain's precision, and so do the four places that restate
// it in hp_kernels.hpp (bdy_gridded, bdy_area, the fused epilogue of godunov_march, the table of godunov_march2): a grid that does not
// cover the interior cells reads outside its buffer.  hp_boundary_add_gridded (hp_actors.hpp) refuses such a grid, by THIS function:
// the kernels' own expression in T, with dx, the offsets and the resolution rounded to T as make_params<T> and area_bdy<T> hand them
// over and the integer coordinate cast as the kernels cast it.  (Checked in double, an fp32 domain took grids whose last column the
// float quotient steps over: dx = 0.3, resolution = 10, 103 columns, off_x = 0.3 gives 2.9999999999999996 in double and 3.0f in float.)
// The expression is monotone in the coordinate -- every operation in it is correctly rounded, hence monotone, and resolution > 0 --
// so the first and the last interior column and row decide for all of them.  Nothing is fused: hp_engine.hip's translation unit is
// built with -ffp-contract=off -fno-fast-math (the Makefile), tests/gridded_probe.cpp likewise.  HIP-free: the probe includes this
// file with a plain host compiler.
#pragma once
#include <cmath>
#include <cstdint>

namespace hp {

// the rain-grid index of model coordinate i along one axis, as the kernels compute it
template <typename T> inline T gridded_index(const long i, const T dx, const T off, const T resolution)
{
	return std::floor((((T)i * dx) - off) / resolution);
}

// one axis: interior coordinates 1 .. n - 2 against a grid of `cells` cells.  For T = double these are the comparisons the check
// has always made (a coordinate left of the grid's origin is refused whatever its quotient rounds to).
template <typename T> inline bool gridded_axis_covers(const T dx, const T off, const T resolution, const long n, const uint64_t cells)
{
	const T lo = ((T)1L * dx) - off;
	if (lo < T(0) || gridded_index<T>(1L, dx, off, resolution) < T(0)) return false;
	if ((double)gridded_index<T>(n - 2, dx, off, resolution) >= (double)cells) return false;
	return true;
}

// 0 <= col < grid_cols at columns 1 and cols - 2, 0 <= row < grid_rows at global rows 1 and global_rows - 2 (a strip's rows are
// global: row_offset is in gy).  The arguments are hp_boundary_add_gridded's and the domain descriptor's, in double as they arrive.
template <typename T> inline bool gridded_covers(const double dx, const double resolution, const double off_x, const double off_y,
                                                 const long cols, const long global_rows, const uint64_t grid_cols, const uint64_t grid_rows)
{
	return gridded_axis_covers<T>((T)dx, (T)off_x, (T)resolution, cols, grid_cols) &&
	       gridded_axis_covers<T>((T)dx, (T)off_y, (T)resolution, global_rows, grid_rows);
}

}  // namespace hp
