// slices_file.hpp -- the `-slices <coord> <bins> <lo> <hi>` flag of nbco3 and nbco: its arguments, and <out>/slices<iter>_<ds>.txt,
// the records of nbco_slice_moments / nbco_2d_slice_moments of one snapshot as text.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../../include/nbco.h"

struct SlicesOpt
{
	bool on = false;
	nbco_hist_axis axis{};
};

// the four values of the flag for a state of `dim` dimensions (x y z vx vy vz; 2-D: x y vx vy), by the rule of the library:
// 1..65536 bins, lo and hi finite, lo < hi.  false: not acceptable
inline bool parse_slices(int dim, const char *coord, const char *bins, const char *lo, const char *hi, SlicesOpt &out)
{
	static const char *const names[6] = {"x", "y", "z", "vx", "vy", "vz"};
	int q = -1;
	for (int a = 0; a < 6; ++a)
		if (std::strcmp(coord, names[a]) == 0 && a % 3 < dim) q = a;
	char *end_bins = nullptr, *end_lo = nullptr, *end_hi = nullptr;
	const long b = std::strtol(bins, &end_bins, 10);   // (saturates on overflow, which the range check then refuses)
	if (q < 0 || end_bins == bins || *end_bins || b < 1 || b > 65536) return false;
	const nbco_hist_axis ax{q, (int)b, std::strtod(lo, &end_lo), std::strtod(hi, &end_hi)};
	if (end_lo == lo || *end_lo || end_hi == hi || *end_hi) return false;
	if (!std::isfinite(ax.lo) || !std::isfinite(ax.hi) || !std::isfinite(ax.hi - ax.lo) || !(ax.lo < ax.hi)) return false;
	out.on = true;
	out.axis = ax;
	return true;
}

// One '#' line naming the columns, one '# outside <k>' line, then per slice: s, its lower edge lo + s (hi - lo) / bins, n, the means,
// then per plane `sig_q sig_p cov_qp emit halo_q halo` -- the columns and the %.17g of moments.txt.  false: the file cannot be written
inline bool write_slices(const std::string &folder, int iter, const std::string &ds, int dim, const nbco_hist_axis &ax, const nbco_moments *rec,
                         long long outside)
{
	static const char *const names[3] = {"x", "y", "z"};
	FILE *f = std::fopen((folder + "/slices" + std::to_string(iter) + '_' + ds + ".txt").c_str(), "w");
	if (!f) return false;
	std::fprintf(f, "# s lo_s n");
	for (int a = 0; a < dim; ++a) std::fprintf(f, " mean_%s", names[a]);
	for (int a = 0; a < dim; ++a) std::fprintf(f, " mean_v%s", names[a]);
	for (int k = 0; k < dim; ++k)
		std::fprintf(f, " sig_%s sig_v%s cov_%s_v%s emit_%s halo_q_%s halo_%s", names[k], names[k], names[k], names[k], names[k], names[k], names[k]);
	std::fprintf(f, "\n# outside %lld\n", outside);
	const double width = (ax.hi - ax.lo) / (double)ax.bins;
	for (int s = 0; s < ax.bins; ++s)
	{
		const nbco_moments &m = rec[s];
		std::fprintf(f, "%d %.17g %lld", s, ax.lo + (double)s * width, m.n);
		for (int a = 0; a < 2 * dim; ++a) std::fprintf(f, " %.17g", m.mean[a]);
		for (int k = 0; k < dim; ++k)
			std::fprintf(f, " %.17g %.17g %.17g %.17g %.17g %.17g", std::sqrt(m.cov[k][k]), std::sqrt(m.cov[dim + k][dim + k]), m.cov[k][dim + k], m.emit[k],
			             m.halo_q[k], m.halo[k]);
		std::fprintf(f, "\n");
	}
	const bool ok = !std::ferror(f);
	return std::fclose(f) == 0 && ok;
}
