// corr_file.hpp -- the `-corr <stride> <frames> <lags>` flag of nbco3 (`-corr-start <iter>`): its arguments, the window of recorded
// frames, and the two files written when the window is full or the run ends: <out>/corr.bin -- the nbco_corr_lag records (64 bytes:
// dx2[3], r4, vv[3] as doubles, pairs as an unsigned 64-bit integer; raw sums) of the lags 0 .. L - 1, L = min(lags, frames recorded)
// -- and <out>/corr.txt, one line `lag tau pairs msd_x msd_y msd_z msd alpha2 vacf_x vacf_y vacf_z` per lag from
// nbco_time_corr_derive, tau = lag * nSteps * dt.  A run that records no frame writes both files empty.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../include/nbco.h"

struct CorrOpt
{
	bool on = false;
	int stride = 1, frames = 0, lags = 0;
	int start = 0;   // the first iteration that may be a frame
};

// the three values of the flag by the rule of the library: stride >= 1, 1 <= lags <= frames <= 2048.  false: not acceptable
inline bool parse_corr(const char *const *v, CorrOpt &out)
{
	long x[3];
	for (int a = 0; a < 3; ++a)
	{
		char *end = nullptr;
		x[a] = std::strtol(v[a], &end, 10);
		if (end == v[a] || *end) return false;
	}
	if (x[0] < 1 || x[0] > 0x7fffffffL || x[2] < 1 || x[2] > x[1] || x[1] > 2048) return false;
	out.on = true;
	out.stride = (int)x[0];
	out.frames = (int)x[1];
	out.lags = (int)x[2];
	return true;
}

// the window of a run: which frame a snapshot iteration fills, and when the files are due
struct CorrWindow
{
	CorrOpt opt;
	long long rows = 0;   // ceil(n / stride) of the particles the run starts with
	int recorded = 0;
	bool written = false;
	CorrWindow(const CorrOpt &opt_, long long n) : opt(opt_), rows(opt_.on ? (n + opt_.stride - 1) / opt_.stride : 0) {}
	// the frame that the snapshot of iteration `iter` fills, or -1
	int frame_for(int iter) const { return opt.on && !written && iter >= opt.start && recorded < opt.frames ? recorded : -1; }
	bool full() const { return opt.on && !written && recorded == opt.frames; }
	int lags() const { return opt.lags < recorded ? opt.lags : recorded; }
	// rec: lags() records.  false: a file cannot be written
	bool write(const std::string &folder, const std::vector<nbco_corr_lag> &rec, double frame_dt)
	{
		written = true;
		std::vector<double> d(8 * rec.size());
		if (!rec.empty() && nbco_time_corr_derive(rec.data(), (int)rec.size(), d.data()) != NBCO_OK) return false;
		FILE *f = std::fopen((folder + "/corr.bin").c_str(), "wb");
		if (!f) return false;
		const bool wrote = std::fwrite(rec.data(), sizeof(nbco_corr_lag), rec.size(), f) == rec.size();
		if (std::fclose(f) != 0 || !wrote) return false;
		FILE *t = std::fopen((folder + "/corr.txt").c_str(), "w");
		if (!t) return false;
		for (size_t l = 0; l < rec.size(); ++l)
		{
			std::fprintf(t, "%zu %.17g %llu", l, (double)l * frame_dt, rec[l].pairs);
			for (int j = 0; j < 8; ++j) std::fprintf(t, " %.17g", d[8 * l + j]);
			std::fprintf(t, "\n");
		}
		return std::fclose(t) == 0;
	}
};
