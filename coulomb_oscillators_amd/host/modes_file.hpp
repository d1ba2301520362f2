// modes_file.hpp -- the `-modes <hx> <hy> <hz> <kx> <ky> <kz> <frames> <lags>` flag of nbco3 (`-modes-start <iter>`): its arguments, the
// window of recorded frames, and the three files written when the window is full or the run ends, for the K wave vectors of the grid
// (the index order of nbco_structure_factor, include/nbco.h) and the lags 0 .. L - 1, L = min(lags, frames recorded):
// <out>/modes.bin -- the K * L nbco_mode_lag records (64 bytes: rr, ll, jj, s0[2], s1[2] as doubles, pairs as an unsigned 64-bit
// integer; raw sums), record (k, lag) at k * L + lag; <out>/modes_derived.bin -- K * L * 4 doubles F F_c C_L C_T from
// nbco_mode_corr_derive with n_norm the mean over the recorded frames of rho.re at k = 0; <out>/modes.txt -- one line
// `ix iy iz |k| F Fc CL CT` per k, at lag 0.  A run that records no frame writes the three files empty.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../include/nbco.h"
#include "sk_file.hpp"

struct ModesOpt
{
	bool on = false;
	nbco_sk_grid g{};
	long long K = 0;
	int frames = 0, lags = 0;
	int start = 0;   // the first iteration that may be a frame
};

// the eight values of the flag by the rule of the library: 0 <= h <= 64, kstep finite and > 0, 1 <= lags <= frames <= 1024.  false: not acceptable
inline bool parse_modes(const char *const *v, ModesOpt &out)
{
	SkOpt grid;
	if (!parse_sk(3, v, grid)) return false;
	long x[2];
	for (int a = 0; a < 2; ++a)
	{
		char *end = nullptr;
		x[a] = std::strtol(v[6 + a], &end, 10);
		if (end == v[6 + a] || *end) return false;
	}
	if (x[1] < 1 || x[1] > x[0] || x[0] > 1024) return false;
	out.on = true;
	out.g = grid.g;
	out.K = grid.K;
	out.frames = (int)x[0];
	out.lags = (int)x[1];
	return true;
}

// the window of a run: which frame a snapshot iteration fills, and when the files are due
struct ModesWindow
{
	ModesOpt opt;
	int recorded = 0;
	bool written = false;
	explicit ModesWindow(const ModesOpt &opt_) : opt(opt_) {}
	// the frame that the snapshot of iteration `iter` fills, or -1
	int frame_for(int iter) const { return opt.on && !written && iter >= opt.start && recorded < opt.frames ? recorded : -1; }
	bool full() const { return opt.on && !written && recorded == opt.frames; }
	int lags() const { return opt.lags < recorded ? opt.lags : recorded; }
	// the index of k = 0
	size_t k0() const { return (size_t)opt.g.h[1] * (size_t)(2 * opt.g.h[2] + 1) + (size_t)opt.g.h[2]; }
	// rec: K * lags() records; rho0: rho.re of the k = 0 record of every recorded frame.  false: a file cannot be written
	bool write(const std::string &folder, const std::vector<nbco_mode_lag> &rec, const std::vector<double> &rho0)
	{
		written = true;
		const int L = lags();
		double n_norm = 0.0;
		for (double r : rho0) n_norm += r;
		if (!rho0.empty()) n_norm /= (double)rho0.size();
		std::vector<double> d(4 * rec.size());
		if (!rec.empty() && nbco_mode_corr_derive(rec.data(), &opt.g, L, n_norm, d.data()) != NBCO_OK) return false;
		FILE *f = std::fopen((folder + "/modes.bin").c_str(), "wb");
		if (!f) return false;
		bool wrote = std::fwrite(rec.data(), sizeof(nbco_mode_lag), rec.size(), f) == rec.size();
		if (std::fclose(f) != 0 || !wrote) return false;
		f = std::fopen((folder + "/modes_derived.bin").c_str(), "wb");
		if (!f) return false;
		wrote = std::fwrite(d.data(), sizeof(double), d.size(), f) == d.size();
		if (std::fclose(f) != 0 || !wrote) return false;
		FILE *t = std::fopen((folder + "/modes.txt").c_str(), "w");
		if (!t) return false;
		const long long ny = 2 * opt.g.h[1] + 1, nz = 2 * opt.g.h[2] + 1;
		for (long long k = 0; L > 0 && k < opt.K; ++k)
		{
			const long long ix = k / (ny * nz), iy = k / nz % ny - opt.g.h[1], iz = k % nz - opt.g.h[2];
			const double kx = (double)ix * opt.g.kstep[0], ky = (double)iy * opt.g.kstep[1], kz = (double)iz * opt.g.kstep[2];
			const double *o = &d[4 * (size_t)k * (size_t)L];
			std::fprintf(t, "%lld %lld %lld %.17g %.17g %.17g %.17g %.17g\n", ix, iy, iz, std::sqrt(kx * kx + ky * ky + kz * kz), o[0], o[1], o[2], o[3]);
		}
		return std::fclose(t) == 0;
	}
};
