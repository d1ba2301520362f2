// sk_file.hpp -- the `-sk` flag of nbco3 (`-sk <hx> <hy> <hz> <kx> <ky> <kz>`) and nbco (`-sk <hx> <hy> <kx> <ky>`): its arguments,
// <out>/sk<iter>_<ds>.bin -- the K pairs of doubles {re, im} of nbco_structure_factor / nbco_2d_structure_factor of one snapshot, in
// the index order of include/nbco.h -- and <out>/sk.txt, one line `iter n_used S_max ix iy iz` per snapshot (2-D: `.. ix iy`): the
// largest |rho_k|^2 / n_used over the k != 0 of the grid and where it sits, from the copied rho on the host, ties to the lowest index.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../include/nbco.h"

struct SkOpt
{
	bool on = false;
	nbco_sk_grid g{};
	long long K = 0;
};

// the 2 dim values of the flag by the rule of the library: 0 <= h <= 64, kstep finite and > 0.  false: not acceptable
inline bool parse_sk(int dim, const char *const *v, SkOpt &out)
{
	nbco_sk_grid g{};
	for (int a = 0; a < dim; ++a)
	{
		char *end_h = nullptr, *end_k = nullptr;
		const long h = std::strtol(v[a], &end_h, 10);
		const double k = std::strtod(v[dim + a], &end_k);
		if (end_h == v[a] || *end_h || h < 0 || h > 64 || end_k == v[dim + a] || *end_k || !std::isfinite(k) || !(k > 0.0)) return false;
		g.h[a] = (int)h;
		g.kstep[a] = k;
	}
	out.on = true;
	out.g = g;
	out.K = (long long)(g.h[0] + 1) * (2 * g.h[1] + 1) * (dim == 3 ? 2 * g.h[2] + 1 : 1);
	return true;
}

struct SkLog
{
	int dim;
	SkOpt opt;
	std::string folder;
	FILE *txt = nullptr;
	SkLog(int dim_, const SkOpt &opt_, const std::string &folder_) : dim(dim_), opt(opt_), folder(folder_)
	{
		if (opt.on) txt = std::fopen((folder + "/sk.txt").c_str(), "w");   // (emptied when the run starts)
	}
	SkLog(const SkLog &) = delete;
	SkLog &operator=(const SkLog &) = delete;
	~SkLog() { if (txt) std::fclose(txt); }
	// rho: 2 K doubles.  false: a file cannot be written
	bool record(int iter, const std::string &ds, const std::vector<double> &rho, long long n_used)
	{
		const int ny = 2 * opt.g.h[1] + 1, nz = dim == 3 ? 2 * opt.g.h[2] + 1 : 1;
		const long long k0 = (long long)opt.g.h[1] * nz + (dim == 3 ? opt.g.h[2] : 0);
		double best = 0.0;
		long long at = k0;
		bool any = false;
		for (long long k = 0; k < opt.K; ++k)
		{
			if (k == k0) continue;
			const double re = rho[2 * (size_t)k], im = rho[2 * (size_t)k + 1], s = n_used > 0 ? (re * re + im * im) / (double)n_used : 0.0;
			if (!any || s > best) { best = s; at = k; any = true; }
		}
		const long long ix = at / ((long long)ny * nz), iy = at / nz % ny - opt.g.h[1], iz = at % nz - (dim == 3 ? opt.g.h[2] : 0);
		bool ok = txt != nullptr;
		if (ok)
		{
			if (dim == 3) std::fprintf(txt, "%d %lld %.17g %lld %lld %lld\n", iter, n_used, best, ix, iy, iz);
			else std::fprintf(txt, "%d %lld %.17g %lld %lld\n", iter, n_used, best, ix, iy);
			ok = std::fflush(txt) == 0;
		}
		FILE *f = std::fopen((folder + "/sk" + std::to_string(iter) + '_' + ds + ".bin").c_str(), "wb");
		if (!f) return false;
		const bool wrote = std::fwrite(rho.data(), sizeof(double), rho.size(), f) == rho.size();
		return std::fclose(f) == 0 && wrote && ok;
	}
};
