// nbco3.cpp -- C++20 host driver over the C ABI (include/nbco.h): the reference's `nbco3` command-line
// interface, initial conditions and headerless binary state files, re-implemented for the MI355X
// engine.  Behaviour follows main3.cu:225-883 (flags :247-623, input :629-652, Gaussian / uniform
// init :71-137,662-666, parameter pack :685-692, -accuracy :737-788, -test :790-811, -test2 :812-831,
// simulation loop + snapshots :832-874).  `-cpu` runs the simulation loop on the host with the compensated direct sum
// (nbco_cpu.hpp: plumbing for small N; the reference's CPU twin of the FMM is out of scope); the test / tuning modes
// need the GPU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <string_view>
#include <vector>

#include "nbco_reference_api.hpp"
#include "nbco_cpu.hpp"
#include "slices_file.hpp"
#include "sk_file.hpp"
#include "corr_file.hpp"
#include "modes_file.hpp"

using namespace nbco_ref;
using namespace std::chrono;

namespace {

#define HIPCHK(call)                                                                                  \
	do {                                                                                              \
		hipError_t e_ = (call);                                                                       \
		if (e_ != hipSuccess) { std::cerr << "GPUassert: " << hipGetErrorString(e_) << ' ' << __FILE__ << ' ' << __LINE__ << std::endl; std::exit((int)e_); } \
	} while (0)

struct V3 { SCAL x, y, z; };

const char *kHelp =
    "This program comes with ABSOLUTELY NO WARRANTY.\n\n"
    "Usage: nbco3 [options] [input]\n\n"
    "  [input] is the path to a binary file with the positions of all particles followed by their\n"
    "  velocities (fp32 xyz triplets, no header).  Without it the system is sampled from a gaussian.\n\n"
    "Other options:\n"
    "  -h or -help       Display this documentation.\n"
    "  -o <output>       Output folder (default './out', must exist).\n"
    "  -n <npart>        Number of particles (default 30001; ignored with [input]).\n"
    "  -ds <v>           Time step (default 5e-4).\n"
    "  -iters <n>        Number of simulation iterations (default 30000).\n"
    "  -steps <n>        Steps between snapshots (default 200).\n"
    "  -integ <name>     Integrator: eu, fr, pefrl (default: leapfrog).\n"
    "  -p <order>        FMM expansion order (default 3).\n"
    "  -r <radius>       Interaction radius (default 1).\n"
    "  -eps <v>          Smoothing length (default 1e-9).\n"
    "  -i <v>            Max FMM level is round(log2(n*i/p^2)) (default 1).\n"
    "  -maxlevel <n>     Maximum kd-tree level.\n"
    "  -ncoll            Skip the P2P pass.\n"
    "  -accuracy <v>     Search r, p for the fastest setting below this error.\n"
    "  -test             Print relative errors and the time of one evaluation.\n"
    "  -test2            Relative error while the tree is reused.\n"
    "  -xi <v>, -omega0 <wx> <wy>, -x <sx> <sy> <sz>, -u <ux> <uy> <uz>   physical parameters.\n"
    "  -snapshot-order <tree|input>   order of the particles in the snapshots: tree (default, as the reference: the order the\n"
    "                    last tree rebuild left them in) or input (every particle keeps the row it had in the initial state).\n"
    "  -energy           At every snapshot append 'iter kinetic elastic coulomb total' to <output>/energy.txt: the Coulomb part from an\n"
    "                    O(N) kd-tree potential pass of its own at the run's -p, -r and -eps (with -cpu: the exact fp64 pair sum).\n"
    "                    The trajectory is not affected; no effect with -test, -test2 or -accuracy.\n"
    "  -moments          At every snapshot append the beam's phase-space moments to <output>/moments.txt (nbco_beam_moments; with -cpu the\n"
    "                    same two-pass fp64 sums on the host): 'iter', the 6 means of (x, y, z, vx, vy, vz), then per plane (x, vx),\n"
    "                    (y, vy), (z, vz) 'sig_q sig_p cov_qp emit halo_q halo'.  The file starts with a '#' line naming the columns.\n"
    "                    The trajectory is not affected; no effect with -test, -test2 or -accuracy.\n"
    "  -slices <x|y|z|vx|vy|vz> <bins> <lo> <hi>   At every snapshot write the moments of -moments per slice along that coordinate\n"
    "                    to <output>/slices<iter>_<ds>.txt (nbco_slice_moments; with -cpu the same bin rule and two-pass sums on the host): a\n"
    "                    particle's slice is the bin (int) ((q - lo) bins / (hi - lo)) of the window lo <= q < hi.  A '#' line names the\n"
    "                    columns, '# outside <k>' counts the particles outside the window, then one line per slice: 's lo_s n', the 6\n"
    "                    means, then per plane 'sig_q sig_p cov_qp emit halo_q halo' of the slice's particles alone (an empty slice: zeros).\n"
    "                    The trajectory is not affected; no effect with -test, -test2 or -accuracy.\n"
    "  -probes <file>    <file> holds probe points (fp32 xyz triplets, no header).  At every snapshot write the field and the potential of\n"
    "                    the charges at these points to <output>/probes<iter>_<ds>.bin: m x 3 doubles of field, then m doubles of\n"
    "                    potential, from a kd-tree walk of its own at the run's -p, -r and -eps (with -cpu: the exact fp64 sums).\n"
    "                    The trajectory is not affected; no effect with -test, -test2 or -accuracy.\n"
    "  -pairs <bins> <rmax>   At every snapshot write the pair statistics of the positions to <output>/pairs<iter>_<ds>.bin: bins + 1\n"
    "                    unsigned 64-bit counts -- the pairs i < j with (b w)^2 <= r^2 < ((b + 1) w)^2, w = rmax / bins, then the pairs with\n"
    "                    r >= rmax -- followed by n doubles: per particle, in the snapshot's order, the squared distance to its nearest\n"
    "                    neighbour below rmax (inf where there is none).  From a range-limited kd-tree walk of its own\n"
    "                    (nbco_pair_hist_tree; with -cpu: all pairs on the host, the same rule, the same bytes).\n"
    "                    The trajectory is not affected; no effect with -test, -test2 or -accuracy.\n"
    "  -bonds <rmax>     At every snapshot write the bond-orientational order of the positions to <output>/bonds<iter>_<ds>.bin: n int32 -- per\n"
    "                    particle, in the snapshot's order, the number of neighbours nb closer than rmax -- then n x 2 doubles: the Steinhardt\n"
    "                    order parameters q4 and q6 of the particle's bonds (0 where nb = 0), and append 'iter bonds isolated nb_max q4_mean\n"
    "                    q6_mean Q4 Q6' to <output>/bonds.txt.  From a range-limited kd-tree walk of its own (nbco_bond_order_tree; with -cpu:\n"
    "                    all pairs on the host, the same neighbour rule and harmonics: the same nb, q to rounding).\n"
    "                    The trajectory is not affected; no effect with -test, -test2 or -accuracy.\n"
    "  -solid <rmax> <dmin> <xi_min>   At every snapshot write which particles are crystalline to <output>/solid<iter>_<ds>.bin: n int32 -- per\n"
    "                    particle, in the snapshot's order, the number of neighbours nb closer than rmax -- then n int32: the number xi of\n"
    "                    those neighbours whose q6 vector is aligned with the particle's own (solid bonds: d6 > dmin), then n x 2 doubles:\n"
    "                    the neighbour-averaged q-bar_4 and q-bar_6 (0 where nb = 0), and append 'iter n_solid solid_bonds xi_max\n"
    "                    qbar4_mean qbar6_mean' to <output>/solid.txt, n_solid the particles with xi >= xi_min.  From one kd-tree of its own\n"
    "                    and two range-limited walks (nbco_bond_solid_tree; with -cpu: all pairs on the host, the same rule: the same nb,\n"
    "                    q-bar to rounding).  The trajectory is not affected; no effect with -test, -test2 or -accuracy.\n"
    "  -sk <hx> <hy> <hz> <kx> <ky> <kz>   At every snapshot write the static structure factor of the positions to <output>/sk<iter>_<ds>.bin:\n"
    "                    K x 2 doubles {re, im} of rho_k = sum_j exp(i k . x_j) on the grid k = (ix kx, iy ky, iz kz), ix = 0..hx, iy = -hy..hy,\n"
    "                    iz = -hz..hz (h <= 64), K = (hx+1)(2hy+1)(2hz+1), at index ((ix)(2hy+1) + iy + hy)(2hz+1) + iz + hz, and append\n"
    "                    'iter n_used S_max ix iy iz' to <output>/sk.txt: the largest |rho_k|^2 / n_used over k != 0 and where it sits\n"
    "                    (nbco_structure_factor; with -cpu the same rule from the same header on the host: equal to rounding).\n"
    "                    The trajectory is not affected; no effect with -test, -test2 or -accuracy.\n"
    "  -corr <stride> <frames> <lags>   Time correlations of individual particles: from the first snapshot iteration >= -corr-start on, every\n"
    "                    snapshot records one frame x y z vx vy vz of the particles number 0, stride, 2 stride, .. (numbers of the initial\n"
    "                    state) until <frames> are in (<= 2048; the frame spacing is the snapshot interval, -steps).  When the window is\n"
    "                    full, or at the end of the run, <output>/corr.bin receives one 64-byte record per lag 0 .. <lags> - 1 (as far as the\n"
    "                    recorded frames allow): the raw sums dx2[3], r4, vv[3] as doubles and the count pairs as a 64-bit integer, over all\n"
    "                    recorded particles and all origins (nbco_time_corr), and <output>/corr.txt one line 'lag tau pairs msd_x msd_y\n"
    "                    msd_z msd alpha2 vacf_x vacf_y vacf_z' per lag, tau = lag * steps * ds: the mean-square displacement, its\n"
    "                    non-Gaussian parameter and the velocity autocorrelation.  A frame is recorded after the aperture and before the\n"
    "                    other outputs; a lost particle's later frames count for nothing.  The flag turns the order tracking of\n"
    "                    '-snapshot-order input' on (the snapshots stay in the order asked for), so leapfrog runs without its fused pass\n"
    "                    between two force evaluations: the same trajectory as with '-snapshot-order input', a slower step.  With -cpu the\n"
    "                    same rule from the same header on the host: pairs equal, the sums to rounding.  Works with -aperture, -bath, -B.\n"
    "                    Refused with -test, -test2 and -accuracy.\n"
    "  -corr-start <iter>   The first iteration that may be a frame of -corr (default 0).\n"
    "  -modes <hx> <hy> <hz> <kx> <ky> <kz> <frames> <lags>   Collective dynamics: from the first snapshot iteration >= -modes-start on, every\n"
    "                    snapshot records the density and current modes rho_k = sum_j exp(i k . x_j), j_k = sum_j v_j exp(i k . x_j) on the\n"
    "                    grid of -sk until <frames> are in (<= 1024; the frame spacing is the snapshot interval, -steps).  When the window is\n"
    "                    full, or at the end of the run, <output>/modes.bin receives one 64-byte record per k and lag 0 .. <lags> - 1 (as far\n"
    "                    as the recorded frames allow; record (k, lag) at k * lags + lag): the raw sums rr, ll, jj, s0[2], s1[2] as doubles\n"
    "                    and pairs as a 64-bit integer (nbco_mode_corr), <output>/modes_derived.bin four doubles F F_c C_L C_T per record --\n"
    "                    the intermediate scattering function, its connected part, the longitudinal and the transverse current correlation\n"
    "                    (nbco_mode_corr_derive, normalised by the mean number of particles that counted) -- and <output>/modes.txt one line\n"
    "                    'ix iy iz |k| F Fc CL CT' per k at lag 0.  A frame is recorded after the aperture and before the other outputs.  No\n"
    "                    particle identity is needed: the order tracking stays as it is and leapfrog keeps its fused pass.  With -cpu the\n"
    "                    frames are summed on the host in index order (equal to rounding) and correlated by nbco_mode_corr_ref.  Works with\n"
    "                    -aperture, -bath, -B.  Refused with -test, -test2 and -accuracy.\n"
    "  -modes-start <iter>   The first iteration that may be a frame of -modes (default 0).\n"
    "  -aperture <ellipsoid|box> <hx> <hy> <hz>   At every snapshot iteration, after the step and before the snapshot, drop the particles\n"
    "                    outside the aperture with these half axes ('inf' opens an axis: pipes, slabs) from the run: they are lost and no\n"
    "                    longer simulated (nbco_aperture_apply; with -cpu the same rule on the host).  Per snapshot\n"
    "                    <output>/lost<iter>_<ds>.bin receives k int32 rows (the rows the lost particles had in the state; with\n"
    "                    -snapshot-order input their particle numbers), then k x 6 floats x y z vx vy vz -- empty when nobody was lost --\n"
    "                    and <output>/losses.txt one line 'iter n_lost n_left'.  The snapshot and -energy, -moments, -probes, -pairs, -bonds, -solid, -sk\n"
    "                    describe the survivors; the snapshot files shrink with n.  A run that loses everybody ends with an error.\n"
    "                    Refused with -test, -test2 and -accuracy.\n"
    "  -aperture-centre <cx> <cy> <cz>   Centre of the aperture (default 0 0 0).\n"
    "  -B <wx> <wy> <wz> Uniform magnetic field Omega = (q/m) B in radians per unit of -ds: the force v x Omega, integrated exactly -- the\n"
    "                    drift of every scheme becomes the motion along a helix (nbco_integrate_steps_b; with -cpu the same matrices and\n"
    "                    arithmetic on the host).  0 0 0 is the run without the flag.  No effect with -test, -test2 or -accuracy.\n"
    "  -bath <gx> <gy> <gz> <Tx> <Ty> <Tz>   Langevin bath: friction rates per unit of -ds and temperatures (units of v^2) per axis; every step is\n"
    "                    wrapped in two exact half steps v <- c1 v + c2 xi of friction and noise (nbco_integrate_steps_t; with -cpu the same\n"
    "                    arithmetic and noise on the host).  A rate of 0 leaves its axis alone, a temperature of 0 is pure cooling; all rates 0\n"
    "                    is the run without the flag.  The step number of an iteration is its tick.  Works with -B, -aperture and -cpu; no\n"
    "                    effect with -test, -test2 or -accuracy.\n"
    "  -bath-seed <u64>  Seed of the bath's noise (default 5351550349027530206, the seed of the reference's initial state).\n"
    "  -cpu              Run the simulation on the host: compensated direct sum O(N^2) over C++20 threads (small N; the test and\n"
    "                    tuning modes need the GPU).  -cpu-threads <n> sets the number of threads (default 8); -cacheline <n> is\n"
    "                    accepted and ignored.\n";

// <folder>/energy.txt of -energy: emptied when the run starts, one line per snapshot
struct EnergyLog
{
	std::ofstream out;
	EnergyLog(bool on, const std::string &folder) { if (on) out.open(folder + "/energy.txt", std::ios::out | std::ios::trunc); }
	void line(int iter, const double (&e)[3])
	{
		if (!out.is_open()) return;
		char buf[160];
		std::snprintf(buf, sizeof buf, "%d %.17g %.17g %.17g %.17g\n", iter, e[0], e[1], e[2], e[0] + e[1] + e[2]);
		out << buf << std::flush;
	}
};

// <folder>/moments.txt of -moments: emptied when the run starts, a '#' line naming the columns, one line per snapshot
struct MomentsLog
{
	std::ofstream out;
	MomentsLog(bool on, const std::string &folder)
	{
		if (!on) return;
		out.open(folder + "/moments.txt", std::ios::out | std::ios::trunc);
		out << "# iter mean_x mean_y mean_z mean_vx mean_vy mean_vz";
		for (const char *k : {"x", "y", "z"})
			out << " sig_" << k << " sig_v" << k << " cov_" << k << "_v" << k << " emit_" << k << " halo_q_" << k << " halo_" << k;
		out << std::endl;
	}
	void line(int iter, const nbco_moments &m)
	{
		if (!out.is_open()) return;
		char buf[64];
		auto put = [&](double v) { std::snprintf(buf, sizeof buf, " %.17g", v); out << buf; };
		out << iter;
		for (int a = 0; a < 6; ++a) put(m.mean[a]);
		for (int k = 0; k < 3; ++k)
		{
			put(std::sqrt(m.cov[k][k])); put(std::sqrt(m.cov[3 + k][3 + k])); put(m.cov[k][3 + k]);
			put(m.emit[k]); put(m.halo_q[k]); put(m.halo[k]);
		}
		out << '\n' << std::flush;
	}
};

// -probes: the points of <file>; false (with a message) for a file that cannot be read, is empty or holds no whole triplets
bool read_probes(const std::string &path, std::vector<float> &pts)
{
	std::ifstream fin(path, std::ios::in | std::ios::binary | std::ios::ate);
	if (!fin) { std::cerr << "Error: cannot read the probe file '" << path << "'" << std::endl; return false; }
	const std::streamoff len = fin.tellg();
	if (len <= 0) { std::cerr << "Error: the probe file '" << path << "' is empty" << std::endl; return false; }
	if (len % 12 != 0) { std::cerr << "Error: the size of the probe file '" << path << "' (" << len << " bytes) is not a multiple of 12 (fp32 xyz triplets)" << std::endl; return false; }
	pts.resize((size_t)len / sizeof(float));
	fin.seekg(0, std::ios::beg);
	fin.read(reinterpret_cast<char *>(pts.data()), (std::streamsize)len);
	if (!fin) { std::cerr << "Error: cannot read the probe file '" << path << "'" << std::endl; return false; }
	return true;
}

// <folder>/probes<iter>_<dt>.bin: out = [field m x 3 | potential m] doubles
bool write_probes(const std::string &folder, int iter, SCAL dt, const std::vector<double> &out)
{
	std::ofstream f(folder + "/probes" + std::to_string(iter) + '_' + std::to_string(dt) + ".bin", std::ios::out | std::ios::binary);
	if (f) f.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)(out.size() * sizeof(double)));
	if (!f) std::cerr << "Error: cannot write the probe file of iteration " << iter << " into \"" << folder << "\"" << std::endl;
	return (bool)f;
}

// -pairs <bins> <rmax> (bins = 0: the flag was not given)
struct PairsOpt
{
	int bins = 0;
	double rmax = 0;
};

// <folder>/pairs<iter>_<dt>.bin: bins + 1 counts, then n doubles of nn2
bool write_pairs(const std::string &folder, int iter, SCAL dt, const std::vector<unsigned long long> &counts, const std::vector<double> &nn2)
{
	std::ofstream f(folder + "/pairs" + std::to_string(iter) + '_' + std::to_string(dt) + ".bin", std::ios::out | std::ios::binary);
	if (f) f.write(reinterpret_cast<const char *>(counts.data()), (std::streamsize)(counts.size() * sizeof(unsigned long long)));
	if (f) f.write(reinterpret_cast<const char *>(nn2.data()), (std::streamsize)(nn2.size() * sizeof(double)));
	if (!f) std::cerr << "Error: cannot write the pair file of iteration " << iter << " into \"" << folder << "\"" << std::endl;
	return (bool)f;
}

// -solid <rmax> <dmin> <xi_min> (rmax = 0: the flag was not given).  <folder>/solid<iter>_<dt>.bin: n int32 of nb, n int32 of xi, then
// n x 2 doubles {q-bar_4, q-bar_6}; <folder>/solid.txt (emptied when the run starts): 'iter n_solid solid_bonds xi_max qbar4_mean
// qbar6_mean' per snapshot
struct SolidOpt
{
	double rmax = 0, dmin = 0;
	int xi_min = 0;
};
struct SolidLog
{
	SolidOpt opt;
	std::string folder;
	std::ofstream out;
	SolidLog(const SolidOpt &opt_, const std::string &folder_) : opt(opt_), folder(folder_)
	{
		if (opt.rmax > 0) out.open(folder + "/solid.txt", std::ios::out | std::ios::trunc);
	}
	bool record(int iter, SCAL dt, const std::vector<int> &nb, const std::vector<int> &xi, const std::vector<double> &qbar, const nbco_solid_summary &s)
	{
		std::ofstream f(folder + "/solid" + std::to_string(iter) + '_' + std::to_string(dt) + ".bin", std::ios::out | std::ios::binary);
		if (f) f.write(reinterpret_cast<const char *>(nb.data()), (std::streamsize)(nb.size() * sizeof(int)));
		if (f) f.write(reinterpret_cast<const char *>(xi.data()), (std::streamsize)(xi.size() * sizeof(int)));
		if (f) f.write(reinterpret_cast<const char *>(qbar.data()), (std::streamsize)(qbar.size() * sizeof(double)));
		char buf[256];
		std::snprintf(buf, sizeof buf, "%d %lld %lld %d %.17g %.17g\n", iter, s.n_solid, s.solid_bonds, s.xi_max, s.qbar_mean[0], s.qbar_mean[1]);
		out << buf << std::flush;
		if (!f || !out) std::cerr << "Error: cannot write the solid files of iteration " << iter << " into \"" << folder << "\"" << std::endl;
		return f && out;
	}
};

// -bonds <rmax> (rmax = 0: the flag was not given).  <folder>/bonds<iter>_<dt>.bin: n int32 of nb, then n x 2 doubles {q4, q6};
// <folder>/bonds.txt (emptied when the run starts): 'iter bonds isolated nb_max q4_mean q6_mean Q4 Q6' per snapshot
struct BondsLog
{
	double rmax;
	std::string folder;
	std::ofstream out;
	BondsLog(double rmax_, const std::string &folder_) : rmax(rmax_), folder(folder_)
	{
		if (rmax > 0) out.open(folder + "/bonds.txt", std::ios::out | std::ios::trunc);
	}
	bool record(int iter, SCAL dt, const std::vector<int> &nb, const std::vector<double> &q, const nbco_bond_summary &s)
	{
		std::ofstream f(folder + "/bonds" + std::to_string(iter) + '_' + std::to_string(dt) + ".bin", std::ios::out | std::ios::binary);
		if (f) f.write(reinterpret_cast<const char *>(nb.data()), (std::streamsize)(nb.size() * sizeof(int)));
		if (f) f.write(reinterpret_cast<const char *>(q.data()), (std::streamsize)(q.size() * sizeof(double)));
		char buf[256];
		std::snprintf(buf, sizeof buf, "%d %lld %lld %d %.17g %.17g %.17g %.17g\n", iter, s.bonds, s.isolated, s.nb_max, s.q_mean[0], s.q_mean[1], s.Q[0], s.Q[1]);
		out << buf << std::flush;
		if (!f || !out) std::cerr << "Error: cannot write the bond files of iteration " << iter << " into \"" << folder << "\"" << std::endl;
		return f && out;
	}
};

// -aperture <shape> <hx> <hy> <hz> and -aperture-centre <cx> <cy> <cz>
struct ApertureOpt
{
	bool on = false;
	nbco_aperture ap{NBCO_AP_ELLIPSOID, {0, 0, 0}, {0, 0, 0}};
};

// <folder>/lost<iter>_<dt>.bin: k int32 ids, then k x 6 floats; <folder>/losses.txt (emptied when the run starts): 'iter n_lost n_left'
struct LossLog
{
	std::ofstream out;
	std::string folder;
	LossLog(bool on, const std::string &folder_) : folder(folder_) { if (on) out.open(folder + "/losses.txt", std::ios::out | std::ios::trunc); }
	bool record(int iter, SCAL dt, const std::vector<int> &ids, const std::vector<float> &recs, long long n_left)
	{
		std::ofstream f(folder + "/lost" + std::to_string(iter) + '_' + std::to_string(dt) + ".bin", std::ios::out | std::ios::binary);
		if (f) f.write(reinterpret_cast<const char *>(ids.data()), (std::streamsize)(ids.size() * sizeof(int)));
		if (f) f.write(reinterpret_cast<const char *>(recs.data()), (std::streamsize)(recs.size() * sizeof(float)));
		out << iter << ' ' << ids.size() << ' ' << n_left << '\n' << std::flush;
		if (!f || !out) std::cerr << "Error: cannot write the loss record of iteration " << iter << " into \"" << folder << "\"" << std::endl;
		return f && out;
	}
};

// `nbco3 -cpu -probes`: the exact sums in fp64 over the fp32 positions, every source at every probe (no self exclusion), eps2 widened
// from float; out = [field m x 3 | potential m]
void cpu_probes(const nbco_cpu::V3 *x, int n, const std::vector<float> &pts, const float *par, float eps2, std::vector<double> &out)
{
	const int m = (int)(pts.size() / 3);
	const float *t = pts.data();
	double *a = out.data(), *psi = out.data() + 3 * (size_t)m;
	const double k = (double)par[0], e = (double)eps2;
	nbco_cpu::for_ranges(m, [=](int lo, int hi) {
		for (int i = lo; i < hi; ++i)
		{
			double ax = 0, ay = 0, az = 0, ps = 0;
			for (int j = 0; j < n; ++j)
			{
				const double dx = (double)t[3 * i] - x[j].x, dy = (double)t[3 * i + 1] - x[j].y, dz = (double)t[3 * i + 2] - x[j].z;
				const double inv = 1.0 / std::sqrt(dx * dx + dy * dy + dz * dz + e), inv3 = inv * inv * inv;
				ps += inv; ax += dx * inv3; ay += dy * inv3; az += dz * inv3;
			}
			a[3 * i] = k * ax; a[3 * i + 1] = k * ay; a[3 * i + 2] = k * az; psi[i] = k * ps;
		}
	});
}

// device allocation that frees itself
template <class T> struct DeviceArray
{
	T *ptr = nullptr;
	explicit DeviceArray(size_t count) { HIPCHK(hipMalloc((void **)&ptr, count * sizeof(T))); }
	~DeviceArray() { if (ptr) (void)hipFree(ptr); }
	DeviceArray(const DeviceArray &) = delete;
	DeviceArray &operator=(const DeviceArray &) = delete;
};

// One run of the program: the device state [pos | vel | acc], the parameter pack and the engine context, with the three
// modes of main3.cu:707-874 as member functions.
struct Session
{
	int n;
	DeviceArray<SCAL> state, par, ref_acc;
	bool have_ref = false;

	Session(const nbco_opts &o, int n_, const std::vector<float> &host, const SCAL (&p)[6]) : n(n_), state(9 * (size_t)n_), par(6), ref_acc(3 * (size_t)n_)
	{
		upload(host);
		HIPCHK(hipMemcpy(par.ptr, p, sizeof p, hipMemcpyHostToDevice));
		init(o);
	}
	~Session() { nbco_destroy(ctx()); ctx() = nullptr; }

	void upload(const std::vector<float> &host) { HIPCHK(hipMemcpy(state.ptr, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice)); }   // acc not copied
	SCAL *acc() { return state.ptr + 6 * (size_t)n; }
	nbco_opts opts() const { nbco_opts cur; nbco_get_opts(ctx(), &cur); return cur; }
	template <class F> void change(F &&f) { nbco_opts cur = opts(); f(cur); init(cur); }

	// seconds per evaluation: one untimed call, then batches of 1, 2, 4, ... calls until min_seconds have passed (main3.cu:707-735)
	SCAL seconds_per_evaluation(SCAL min_seconds)
	{
		compute_force(fmm_cart3_kdtree, state.ptr, n, par.ptr);
		long long calls = 0;
		SCAL elapsed = 0;
		const auto t0 = steady_clock::now();
		for (long long batch = 1; calls == 0 || elapsed < min_seconds; batch *= 2)
		{
			for (long long i = 0; i < batch; ++i) compute_force(fmm_cart3_kdtree, state.ptr, n, par.ptr);
			calls += batch;
			elapsed = duration_cast<microseconds>(steady_clock::now() - t0).count() * (SCAL)1.e-6;
		}
		return elapsed / (SCAL)calls;
	}

	// mean relative error of the FMM accelerations against the compensated direct sum (main3.cu:139-181).  With the caller's
	// order kept (unsort) the direct sum is cached until `refresh`; otherwise the FMM runs first because it permutes the state.
	SCAL mean_error(bool refresh)
	{
		float err = 0;
		if (opts().unsort)
		{
			if (refresh || !have_ref)
			{
				compute_force(direct3, state.ptr, n, par.ptr);
				check(nbco_copy(ctx(), ref_acc.ptr, acc(), n), "copy");
				have_ref = true;
			}
			compute_force(fmm_cart3_kdtree, state.ptr, n, par.ptr);
			check(nbco_mean_relerr(ctx(), acc(), ref_acc.ptr, n, &err), "mean_relerr");
		}
		else
		{
			compute_force(fmm_cart3_kdtree, state.ptr, n, par.ptr);
			check(nbco_copy(ctx(), ref_acc.ptr, acc(), n), "copy");
			compute_force(direct3, state.ptr, n, par.ptr);
			check(nbco_mean_relerr(ctx(), ref_acc.ptr, acc(), n, &err), "mean_relerr");
		}
		return (SCAL)err;
	}

	// -accuracy: fastest (r, p) of the grid of main3.cu:739-740 whose error stays below the bound (main3.cu:737-788)
	int search_parameters(SCAL bound)
	{
		struct Candidate { SCAL r; int p; SCAL seconds, error; };
		static constexpr SCAL radii[] = {1.11f, 1.25f, 1.43f, 1.67f, 2.f, 2.5f, 3.f};
		std::vector<Candidate> admissible;
		std::cout << "Parameter optimization in progress, please wait" << std::flush;
		for (SCAL r : radii)
			for (int p = 1; p <= 6; ++p)
			{
				change([&](nbco_opts &c) { c.coll = 1; c.unsort = 1; c.tree_radius = r; c.fmm_order = p; });
				const SCAL e = mean_error(false);
				if (e < bound) admissible.push_back({r, p, seconds_per_evaluation(0), e});
				std::cout << '.' << std::flush;
			}
		if (admissible.empty()) { std::cout << "\nOptimization failed!" << std::endl; return -1; }
		const Candidate *best = &admissible.front();
		for (const Candidate &c : admissible)
			if (c.seconds < best->seconds) best = &c;
		change([&](nbco_opts &c) { c.tree_radius = best->r; c.fmm_order = best->p; });
		std::cout << "\nBest parameters: r = " << best->r << ", p = " << best->p << ", time = " << best->seconds << ", error = " << best->error << std::endl;
		return 0;
	}

	// -test: time of one evaluation at the chosen order, then the error table for orders 1..10 (main3.cu:790-811)
	void print_error_table(const std::vector<float> &host)
	{
		change([](nbco_opts &c) { c.unsort = 0; });
		std::cout << opts().fmm_order << ": Average time: " << seconds_per_evaluation(1) << " [s]" << std::endl;
		upload(host);   // the timing loop permuted the state: the table is quoted in the caller's order
		for (int p = 1; p <= 10; ++p)
		{
			change([&](nbco_opts &c) { c.unsort = 1; c.fmm_order = p; });
			std::cout << p << ": Relative error: " << mean_error(p == 1) << std::endl;
		}
	}

	// -test2: error of successive evaluations while the particles move in the trap and the tree is reused (main3.cu:812-831)
	void print_reuse_errors(SCAL dt)
	{
		change([](nbco_opts &c) { c.unsort = 0; });
		const int evaluations = opts().tree_steps + 1;
		for (int i = 0; i < evaluations; ++i)
		{
			const SCAL e = mean_error(false);
			pre_symplectic_euler(add_elastic, state.ptr, n, par.ptr + 3, dt, step);
			std::cout << "Relative error after " << i << " steps: " << e << std::endl;
		}
	}

	// simulation: accelerations first, then nIters fused integrator steps; a snapshot [pos | vel] every nSteps iterations
	// (main3.cu:832-874).  Evaluations are enqueued without a drain; the copy of a snapshot is what waits for the device.
	int simulate(int scheme, SCAL dt, int nIters, int nSteps, const std::string &folder, std::vector<float> &host, size_t state_bytes, bool input_order,
	             bool energy, bool moments, const std::vector<float> &probes, const PairsOpt &pairs, double bonds_rmax, const SolidOpt &solid, const SkOpt &sk, const ApertureOpt &aperture,
	             const SlicesOpt &slices, const double *omega, const nbco_bath &bath, const CorrOpt &corr, const ModesOpt &modes)
	{
		// -modes: the series of mode records on the device (K x frames x 8 doubles) and the records of the lags
		ModesWindow mwin(modes);
		DeviceArray<double> modes_series(modes.on ? (size_t)modes.K * (size_t)modes.frames * 8 : 0);
		DeviceArray<nbco_mode_lag> modes_out(modes.on ? (size_t)modes.K * (size_t)modes.lags : 0);
		auto modes_finish = [&]() {
			std::vector<nbco_mode_lag> rec((size_t)modes.K * (size_t)mwin.lags());
			std::vector<double> row((size_t)mwin.recorded * 8), rho0;
			if (!rec.empty())
			{
				check(nbco_mode_corr(ctx(), modes_series.ptr, &modes.g, modes.frames, mwin.recorded, mwin.lags(), modes_out.ptr), "mode_corr");
				check(nbco_sync(ctx()), "sync");
				HIPCHK(hipMemcpy(rec.data(), modes_out.ptr, rec.size() * sizeof(nbco_mode_lag), hipMemcpyDeviceToHost));
				HIPCHK(hipMemcpy(row.data(), modes_series.ptr + mwin.k0() * (size_t)modes.frames * 8, row.size() * sizeof(double), hipMemcpyDeviceToHost));
				for (int f = 0; f < mwin.recorded; ++f) rho0.push_back(row[8 * (size_t)f]);
			}
			if (mwin.write(folder, rec, rho0)) return true;
			std::cerr << "Error: cannot write the modes files into \"" << folder << "\"" << std::endl;
			return false;
		};
		// -corr: the window of frames on the device (rows by the particles the run starts with) and the records of the lags
		CorrWindow cwin(corr, n);
		DeviceArray<float> corr_traj(corr.on ? (size_t)cwin.rows * (size_t)corr.frames * 6 : 0);
		DeviceArray<nbco_corr_lag> corr_out(corr.on ? (size_t)corr.lags : 0);
		auto corr_finish = [&]() {
			std::vector<nbco_corr_lag> rec((size_t)cwin.lags());
			if (!rec.empty())
			{
				check(nbco_time_corr(ctx(), corr_traj.ptr, cwin.rows, corr.frames, cwin.recorded, cwin.lags(), corr_out.ptr), "time_corr");
				check(nbco_sync(ctx()), "sync");
				HIPCHK(hipMemcpy(rec.data(), corr_out.ptr, rec.size() * sizeof(nbco_corr_lag), hipMemcpyDeviceToHost));
			}
			if (cwin.write(folder, rec, (double)nSteps * (double)dt)) return true;
			std::cerr << "Error: cannot write the correlation files into \"" << folder << "\"" << std::endl;
			return false;
		};
		std::vector<nbco_moments> slice_recs(slices.on ? (size_t)slices.axis.bins : 0);
		// -aperture: the loss record on the device (room for everybody) and the host copies that go into the files
		const size_t ap_n = aperture.on ? (size_t)n : 0;
		DeviceArray<float> lost_dev(6 * ap_n);
		DeviceArray<int> lost_row_dev(ap_n);
		std::vector<float> lost_recs;
		std::vector<int> lost_ids, rank;
		bool sparse = false;   // -snapshot-order input: somebody has been lost, the particle numbers of the state have gaps
		LossLog llog(aperture.on, folder);
		// -pairs: the counts and nn2 on the device, and the host copies that go into the files
		const size_t pair_n = pairs.bins ? (size_t)n : 0, pair_c = pairs.bins ? (size_t)pairs.bins + 1 : 0;
		DeviceArray<unsigned long long> pairs_counts(pair_c);
		DeviceArray<double> pairs_nn2(pair_n);
		std::vector<unsigned long long> pairs_counts_host(pair_c);
		std::vector<double> pairs_nn2_host(pair_n), pairs_rows(input_order ? pair_n : 0);
		// -bonds: nb and {q4, q6} on the device, and the host copies that go into the files
		const size_t bond_n = bonds_rmax > 0 ? (size_t)n : 0;
		DeviceArray<int> bonds_nb(bond_n);
		DeviceArray<double> bonds_q(2 * bond_n);
		std::vector<int> bonds_nb_host(bond_n), bonds_nb_rows(input_order ? bond_n : 0);
		std::vector<double> bonds_q_host(2 * bond_n), bonds_q_rows(input_order ? 2 * bond_n : 0);
		BondsLog blog(bonds_rmax, folder);
		// -solid: nb, xi and {q-bar_4, q-bar_6} on the device, and the host copies that go into the files
		const size_t solid_n = solid.rmax > 0 ? (size_t)n : 0;
		DeviceArray<int> solid_nb(solid_n), solid_xi(solid_n);
		DeviceArray<double> solid_q(2 * solid_n);
		std::vector<int> solid_nb_host(solid_n), solid_xi_host(solid_n), solid_nb_rows(input_order ? solid_n : 0), solid_xi_rows(input_order ? solid_n : 0);
		std::vector<double> solid_q_host(2 * solid_n), solid_q_rows(input_order ? 2 * solid_n : 0);
		SolidLog slog(solid, folder);
		// -sk: rho on the device and the host copy that goes into the file
		DeviceArray<double> sk_rho(sk.on ? 2 * (size_t)sk.K : 0);
		std::vector<double> sk_rho_host(sk.on ? 2 * (size_t)sk.K : 0);
		SkLog sklog(3, sk, folder);
		EnergyLog elog(energy, folder);
		MomentsLog mlog(moments, folder);
		// -probes: the points and their results [field m x 3 | potential m] on the device, and the host copy that goes into the files
		const size_t m = probes.size() / 3;
		DeviceArray<float> probes_dev(probes.size());   // (nothing is allocated without the flag)
		DeviceArray<double> probes_out(4 * m);
		std::vector<double> probes_host(4 * m);
		if (m) HIPCHK(hipMemcpy(probes_dev.ptr, probes.data(), probes.size() * sizeof(float), hipMemcpyHostToDevice));
		change([&](nbco_opts &c) { c.unsort = 0; c.sync = 0; c.track_order = input_order || corr.on ? 1 : 0; });
		std::vector<int> order(input_order ? (size_t)n : 0);
		std::vector<float> rows(input_order ? host.size() : 0);
		check(nbco_force(ctx(), NBCO_EVAL_FMM_KDTREE, state.ptr, n, par.ptr, 1), "compute_force");
		check(nbco_sync(ctx()), "sync");
		auto loop_t0 = std::chrono::steady_clock::now(), steady_t0 = loop_t0;
		int loop_first = 0, steady_first = -1;
		// (not in the reference: a second clock that starts kSteadyFrom iterations in, behind the first builds of the run -- cold
		// median selections, list buffers sized from nothing -- so that the figure is comparable with a library run in its stride)
		constexpr int kSteadyFrom = 9;
		// snapshots follow the iterations 0, nSteps, 2 nSteps, ..: the steps in between are ONE nbco_integrate_steps call (same final
		// state as step-by-step calls; leapfrog fuses what lies between two force evaluations into one pass)
		for (int iter = 0; iter < nIters;)
		{
			int run = iter % nSteps == 0 ? 1 : std::min(nSteps - iter % nSteps, nIters - iter);
			if (steady_first < 0 && nIters >= 3 * kSteadyFrom)
			{
				if (iter == kSteadyFrom) { check(nbco_sync(ctx()), "sync"); steady_t0 = std::chrono::steady_clock::now(); steady_first = iter; }
				else if (iter < kSteadyFrom) run = std::min(run, kSteadyFrom - iter);   // (K steps in one call == the same steps in two calls, bit for bit)
			}
			// (omega null and all rates zero: the library makes this the plain nbco_integrate_steps call)
			check(nbco_integrate_steps_t(ctx(), scheme, NBCO_EVAL_FMM_KDTREE, state.ptr, n, par.ptr, (double)dt, 1.0, 1, run, omega, &bath, (unsigned long long)iter), "integrate");
			iter += run;
			if ((iter - 1) % nSteps != 0) continue;
			const int snap = iter - 1;
			std::cout << snap << ' ' << std::flush;
			check(nbco_sync(ctx()), "sync");
			// the engine composes the permutations of all tree rebuilds: row i of the state is particle order[i] of the initial state
			if (input_order) check(nbco_kd_copy(ctx(), NBCO_KD_ORDER, order.data(), (long long)(order.size() * sizeof(int))), "kd_copy");
			if (aperture.on)
			{
				// the lost particles leave the state on the device: [pos n | vel n | acc n] -> [pos n' | vel n' | acc n'], order kept
				long long kept = 0;
				check(nbco_aperture_apply(ctx(), state.ptr, n, &aperture.ap, &kept, lost_dev.ptr, lost_row_dev.ptr, (long long)n), "aperture_apply");
				const size_t k = (size_t)(n - kept);
				lost_ids.resize(k);
				lost_recs.resize(6 * k);
				if (k)
				{
					HIPCHK(hipMemcpy(lost_ids.data(), lost_row_dev.ptr, k * sizeof(int), hipMemcpyDeviceToHost));
					HIPCHK(hipMemcpy(lost_recs.data(), lost_dev.ptr, 6 * k * sizeof(float), hipMemcpyDeviceToHost));
				}
				if (input_order && k)
				{
					// particle numbers instead of rows; the lost entries leave the host copy of the order map as they left the engine's
					size_t next = 0, w = 0;
					for (size_t i = 0; i < (size_t)n; ++i)
					{
						if (next < k && (size_t)lost_ids[next] == i) lost_ids[next++] = order[i];
						else order[w++] = order[i];
					}
					order.resize(w);
					sparse = true;
				}
				n = (int)kept;
				state_bytes = 6 * (size_t)n * sizeof(float);
				host.resize(6 * (size_t)n);
				if (!llog.record(snap, dt, lost_ids, lost_recs, kept)) return -1;
				if (n == 0)
				{
					std::cerr << "\nError: every particle is outside the aperture at iteration " << snap << ": nothing is left to simulate" << std::endl;
					return -1;
				}
			}
			if (const int frame = cwin.frame_for(snap); frame >= 0)
			{
				// through the engine's order map, on the device: row i of the state goes to the row of its particle number
				check(nbco_traj_record(ctx(), state.ptr, n, nullptr, corr_traj.ptr, cwin.rows, corr.frames, frame, corr.stride), "traj_record");
				++cwin.recorded;
				if (cwin.full() && !corr_finish()) return -1;
			}
			if (const int frame = mwin.frame_for(snap); frame >= 0)
			{
				// sums over the particles: the order of the state does not matter to them
				check(nbco_modes_record(ctx(), state.ptr, n, &modes.g, modes_series.ptr, modes.frames, frame, nullptr), "modes_record");
				++mwin.recorded;
				if (mwin.full() && !modes_finish()) return -1;
			}
			HIPCHK(hipMemcpy(host.data(), state.ptr, state_bytes, hipMemcpyDeviceToHost));   // acc not copied
			std::ofstream fout(folder + "/out" + std::to_string(snap) + '_' + std::to_string(dt) + ".bin", std::ios::out | std::ios::binary);
			if (!fout)
			{
				std::cerr << "Error: cannot write on output location. Check that \"" << folder << "\" folder exists. Create it if not." << std::endl;
				return -1;
			}
			if (input_order)
			{
				// rank[r]: the state row that goes into row r of the file -- the particles in increasing particle number, which is the
				// inverse of the order map while nobody is lost and a sort by the (sparse) numbers afterwards
				rank.resize((size_t)n);
				if (!sparse)
					for (size_t i = 0; i < (size_t)n; ++i) rank[(size_t)order[i]] = (int)i;
				else
				{
					for (size_t i = 0; i < (size_t)n; ++i) rank[i] = (int)i;
					std::sort(rank.begin(), rank.end(), [&](int a, int b) { return order[(size_t)a] < order[(size_t)b]; });
				}
				for (size_t r = 0; r < (size_t)n; ++r)
					for (int k = 0; k < 3; ++k)
					{
						rows[3 * r + k] = host[3 * (size_t)rank[r] + k];
						rows[3 * ((size_t)n + r) + k] = host[3 * ((size_t)n + rank[r]) + k];
					}
				fout.write(reinterpret_cast<const char *>(rows.data()), (std::streamsize)state_bytes);
			}
			else fout.write(reinterpret_cast<const char *>(host.data()), (std::streamsize)state_bytes);
			if (energy)
			{
				// a tree of its own on a private context: the run's tree, rebuild schedule and state are not touched
				double e3[3];
				check(nbco_energy_tree(ctx(), state.ptr, n, par.ptr, e3, nullptr), "energy_tree");
				elog.line(snap, e3);
			}
			if (moments)
			{
				// two reduction passes over the state as it is; they use only the transient reduction scratch of the context
				nbco_moments mom;
				check(nbco_beam_moments(ctx(), state.ptr, n, &mom), "beam_moments");
				mlog.line(snap, mom);
			}
			if (slices.on)
			{
				// grouped by slice in scratch of the call's own: the state and the run's tree are not touched
				long long outside = 0;
				check(nbco_slice_moments(ctx(), state.ptr, n, &slices.axis, slice_recs.data(), &outside), "slice_moments");
				if (!write_slices(folder, snap, std::to_string(dt), 3, slices.axis, slice_recs.data(), outside))
				{
					std::cerr << "Error: cannot write the slice file of iteration " << snap << " into \"" << folder << "\"" << std::endl;
					return -1;
				}
			}
			if (m)
			{
				// the same private context: a tree over a scratch copy of the positions, walked by the probes
				check(nbco_probe_tree(ctx(), state.ptr, n, probes_dev.ptr, (long long)m, par.ptr, probes_out.ptr, probes_out.ptr + 3 * m), "probe_tree");
				check(nbco_sync(ctx()), "sync");
				HIPCHK(hipMemcpy(probes_host.data(), probes_out.ptr, probes_host.size() * sizeof(double), hipMemcpyDeviceToHost));
				if (!write_probes(folder, snap, dt, probes_host)) return -1;
			}
			if (pairs.bins)
			{
				// the same private context: a tree over a scratch copy of the positions, walked by the particles themselves
				check(nbco_pair_hist_tree(ctx(), state.ptr, n, pairs.bins, pairs.rmax, pairs_counts.ptr, pairs_nn2.ptr), "pair_hist_tree");
				check(nbco_sync(ctx()), "sync");
				HIPCHK(hipMemcpy(pairs_counts_host.data(), pairs_counts.ptr, pair_c * sizeof(unsigned long long), hipMemcpyDeviceToHost));
				pairs_nn2_host.resize((size_t)n);
				HIPCHK(hipMemcpy(pairs_nn2_host.data(), pairs_nn2.ptr, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
				if (input_order)
				{
					pairs_rows.resize((size_t)n);
					for (size_t r = 0; r < (size_t)n; ++r) pairs_rows[r] = pairs_nn2_host[(size_t)rank[r]];   // (the rows of the snapshot file)
					if (!write_pairs(folder, snap, dt, pairs_counts_host, pairs_rows)) return -1;
				}
				else if (!write_pairs(folder, snap, dt, pairs_counts_host, pairs_nn2_host)) return -1;
			}
			if (bonds_rmax > 0)
			{
				// the same private context and the same walk, with the harmonics of the bonds at the leaves; the summary synchronises
				nbco_bond_summary bsum;
				check(nbco_bond_order_tree(ctx(), state.ptr, n, bonds_rmax, bonds_nb.ptr, bonds_q.ptr, &bsum), "bond_order_tree");
				bonds_nb_host.resize((size_t)n);
				bonds_q_host.resize(2 * (size_t)n);
				HIPCHK(hipMemcpy(bonds_nb_host.data(), bonds_nb.ptr, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
				HIPCHK(hipMemcpy(bonds_q_host.data(), bonds_q.ptr, 2 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
				if (input_order)
				{
					bonds_nb_rows.resize((size_t)n);
					bonds_q_rows.resize(2 * (size_t)n);
					for (size_t r = 0; r < (size_t)n; ++r)   // (the rows of the snapshot file)
					{
						bonds_nb_rows[r] = bonds_nb_host[(size_t)rank[r]];
						bonds_q_rows[2 * r] = bonds_q_host[2 * (size_t)rank[r]];
						bonds_q_rows[2 * r + 1] = bonds_q_host[2 * (size_t)rank[r] + 1];
					}
					if (!blog.record(snap, dt, bonds_nb_rows, bonds_q_rows, bsum)) return -1;
				}
				else if (!blog.record(snap, dt, bonds_nb_host, bonds_q_host, bsum)) return -1;
			}
			if (solid.rmax > 0)
			{
				// one call: the private context's tree, the walk of the harmonics and the walk of the records; the summary synchronises
				nbco_solid_summary ssum;
				check(nbco_bond_solid_tree(ctx(), state.ptr, n, solid.rmax, nullptr, solid.dmin, solid.xi_min, solid_nb.ptr, solid_xi.ptr, solid_q.ptr, &ssum), "bond_solid_tree");
				solid_nb_host.resize((size_t)n);
				solid_xi_host.resize((size_t)n);
				solid_q_host.resize(2 * (size_t)n);
				HIPCHK(hipMemcpy(solid_nb_host.data(), solid_nb.ptr, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
				HIPCHK(hipMemcpy(solid_xi_host.data(), solid_xi.ptr, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
				HIPCHK(hipMemcpy(solid_q_host.data(), solid_q.ptr, 2 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
				if (input_order)
				{
					solid_nb_rows.resize((size_t)n);
					solid_xi_rows.resize((size_t)n);
					solid_q_rows.resize(2 * (size_t)n);
					for (size_t r = 0; r < (size_t)n; ++r)   // (the rows of the snapshot file)
					{
						solid_nb_rows[r] = solid_nb_host[(size_t)rank[r]];
						solid_xi_rows[r] = solid_xi_host[(size_t)rank[r]];
						solid_q_rows[2 * r] = solid_q_host[2 * (size_t)rank[r]];
						solid_q_rows[2 * r + 1] = solid_q_host[2 * (size_t)rank[r] + 1];
					}
					if (!slog.record(snap, dt, solid_nb_rows, solid_xi_rows, solid_q_rows, ssum)) return -1;
				}
				else if (!slog.record(snap, dt, solid_nb_host, solid_xi_host, solid_q_host, ssum)) return -1;
			}
			if (sk.on)
			{
				// a sum over the particles: the order of the state does not matter to it
				long long n_used = 0;
				check(nbco_structure_factor(ctx(), state.ptr, n, &sk.g, sk_rho.ptr, &n_used), "structure_factor");
				HIPCHK(hipMemcpy(sk_rho_host.data(), sk_rho.ptr, sk_rho_host.size() * sizeof(double), hipMemcpyDeviceToHost));
				if (!sklog.record(snap, std::to_string(dt), sk_rho_host, n_used))
				{
					std::cerr << "Error: cannot write the structure factor files of iteration " << snap << " into \"" << folder << "\"" << std::endl;
					return -1;
				}
			}
			if (snap == 0) { loop_t0 = std::chrono::steady_clock::now(); loop_first = 1; }   // the timer below starts behind the first snapshot
		}
		check(nbco_sync(ctx()), "sync");
		if (corr.on && !cwin.written && !corr_finish()) return -1;
		if (modes.on && !mwin.written && !modes_finish()) return -1;
		std::cout << std::endl;
		// (not in the reference: wall time of the integration loop behind the first snapshot -- what bench.py's `cli` leg reads)
		const auto loop_t1 = std::chrono::steady_clock::now();
		std::cout << "Loop time: " << std::chrono::duration<double>(loop_t1 - loop_t0).count() << " s, " << nIters - loop_first << " iterations" << std::endl;
		if (steady_first >= 0)
			std::cout << "Steady loop time: " << std::chrono::duration<double>(loop_t1 - steady_t0).count() << " s, " << nIters - steady_first
			          << " iterations (from iteration " << steady_first << " on)" << std::endl;
		return 0;
	}
};

} // namespace

int main(int argc, const char **argv)
{
	std::cout << "N-body coulomb oscillators -- MI355X engine (nbco3 interface of locuoco/coulomb_oscillators)\n\n"
	             "Type 'nbco3 -h' for a brief documentation.\n\n";

	int nBodies = 30001;
	SCAL dt = (SCAL)5.e-4;
	int nIters = 30001, nSteps = 200;
	std::string strout("out"), strin, strprobes;
	std::vector<float> probes;
	PairsOpt pairs;
	double bonds_rmax = 0;
	SolidOpt solid;
	SkOpt sk;
	CorrOpt corr;
	ModesOpt modes;
	ApertureOpt aperture;
	SlicesOpt slices;
	bool in = false, test = false, test2 = false, b_accuracy = false, input_order = false, cpu = false, energy = false, moments = false, bfield = false;
	double omega_b[3]{0, 0, 0};
	nbco_bath bath{{0, 0, 0}, {0, 0, 0}, NBCO_REF_SEED};
	bool bath_on = false;
	SCAL accuracy = (SCAL)0.001;
	int scheme = NBCO_INTEG_LEAPFROG;   // main3.cu:238
	SCAL xi = (SCAL)2.e-6;
	V3 omega0{(SCAL)1.095, (SCAL)1.0, (SCAL)1.0}, x{(SCAL)0.003, (SCAL)0.001, (SCAL)0.01};
	V3 u{omega0.x * x.x, omega0.y * x.y, omega0.z * x.z};
	nbco_opts o;
	nbco_opts_default(&o);
	o.tree_steps = 8;    // constants.cuh:45, the reference GPU driver's rebuild cadence
	o.m2l_first = 1;     // reference GPU traversal order (fmm_cart3_kdtree.cuh:520-534)

	auto need = [&](int i, int k, const char *flag) {
		if (i + k >= argc) { std::cerr << "Error: missing argument" << (k > 1 ? "(s)" : "") << " to '" << flag << "'\n"; return false; }
		return true;
	};
	for (int i = 1; i < argc; ++i)
	{
		std::string_view a(argv[i]);
		if (a.empty() || a[0] != '-') { strin = argv[i]; in = true; continue; }
		if (a == "-h" || a == "-help") { std::cout << kHelp; return 0; }
		else if (a == "-o") { if (!need(i, 1, "-o")) return -1; strout = argv[++i]; }
		else if (a == "-n")
		{
			if (!need(i, 1, "-n")) return -1;
			nBodies = atoi(argv[i + 1]);
			if (nBodies <= 0) { std::cerr << "Error: invalid argument to '-n': " << argv[i + 1] << '\n'; return -1; }
			++i;
		}
		else if (a == "-ds")
		{
			if (!need(i, 1, "-ds")) return -1;
			dt = (SCAL)atof(argv[i + 1]);
			if (dt <= 0) { std::cerr << "Error: invalid argument to '-ds': " << argv[i + 1] << '\n'; return -1; }
			++i;
		}
		else if (a == "-iters")
		{
			if (!need(i, 1, "-iters")) return -1;
			nIters = atoi(argv[i + 1]) + 1;   // main3.cu:357
			if (nIters <= 0) { std::cerr << "Error: invalid argument to '-iters': " << argv[i + 1] << '\n'; return -1; }
			++i;
		}
		else if (a == "-steps")
		{
			if (!need(i, 1, "-steps")) return -1;
			nSteps = atoi(argv[i + 1]);
			if (nSteps <= 0) { std::cerr << "Error: invalid argument to '-steps': " << argv[i + 1] << '\n'; return -1; }
			++i;
		}
		else if (a == "-integ")
		{
			if (!need(i, 1, "-integ")) return -1;
			// the reference compares from the second character on (main3.cu:389-395): "-fr", "xfr", ...;
			// the documented bare names are accepted as well
			std::string_view v(argv[i + 1]);
			std::string_view tail = v.size() > 1 ? v.substr(1) : std::string_view{};
			if (v == "eu" || tail == "eu") scheme = NBCO_INTEG_EULER;
			else if (v == "fr" || tail == "fr") scheme = NBCO_INTEG_FORESTRUTH;
			else if (v == "pefrl" || tail == "pefrl") scheme = NBCO_INTEG_PEFRL;
			else { std::cerr << "Error: invalid argument to '-integ': " << argv[i + 1] << '\n'; return -1; }
			++i;
		}
		else if (a == "-p")
		{
			if (!need(i, 1, "-p")) return -1;
			o.fmm_order = atoi(argv[i + 1]);
			if (o.fmm_order <= 0) { std::cerr << "Error: invalid argument to '-p': " << argv[i + 1] << '\n'; return -1; }
			++i;
		}
		else if (a == "-r")
		{
			if (!need(i, 1, "-r")) return -1;
			o.tree_radius = (float)atof(argv[i + 1]);
			if (o.tree_radius <= 0) { std::cerr << "Error: invalid argument to '-r': " << argv[i + 1] << '\n'; return -1; }
			++i;
		}
		else if (a == "-eps")
		{
			if (!need(i, 1, "-eps")) return -1;
			float e = (float)atof(argv[i + 1]);
			if (e <= 0) { std::cerr << "Error: invalid argument to '-eps': " << argv[i + 1] << '\n'; return -1; }
			o.eps2 = e * e;   // main3.cu:440-446
			if (o.eps2 == 0) { std::cerr << "Error: too small argument to '-eps': " << argv[i + 1] << '\n'; return -1; }
			++i;
		}
		else if (a == "-i")
		{
			if (!need(i, 1, "-i")) return -1;
			o.dens_inhom = (float)atof(argv[i + 1]);
			if (o.dens_inhom <= 0) { std::cerr << "Error: invalid argument to '-i': " << argv[i + 1] << " (should be greater than 0)\n"; return -1; }
			++i;
		}
		else if (a == "-maxlevel")
		{
			if (!need(i, 1, "-maxlevel")) return -1;
			o.tree_L = atoi(argv[i + 1]);
			if (o.tree_L <= 0) { std::cerr << "Error: invalid argument to '-maxlevel': " << argv[i + 1] << " (should be greater than 0)\n"; return -1; }
			++i;
		}
		else if (a == "-ncoll") o.coll = 0;
		else if (a == "-accuracy")
		{
			if (!need(i, 1, "-accuracy")) return -1;
			b_accuracy = true;
			accuracy = (SCAL)atof(argv[i + 1]);
			if (accuracy <= 0) { std::cerr << "Error: invalid argument to '-accuracy': " << argv[i + 1] << " (should be greater than 0)\n"; return -1; }
			++i;
		}
		else if (a == "-cpu") cpu = true;
		else if (a == "-energy") energy = true;
		else if (a == "-moments") moments = true;
		else if (a == "-slices")
		{
			if (!need(i, 4, "-slices")) return -1;
			if (!parse_slices(3, argv[i + 1], argv[i + 2], argv[i + 3], argv[i + 4], slices))
			{
				std::cerr << "Error: invalid argument(s) to '-slices': " << argv[i + 1] << ' ' << argv[i + 2] << ' ' << argv[i + 3] << ' ' << argv[i + 4]
				          << " (x, y, z, vx, vy or vz, 1..65536 bins, lo below hi, both finite)\n";
				return -1;
			}
			i += 4;
		}
		else if (a == "-probes")
		{
			if (!need(i, 1, "-probes")) return -1;
			strprobes = argv[++i];
			if (!read_probes(strprobes, probes)) return -1;
		}
		else if (a == "-pairs")
		{
			if (!need(i, 2, "-pairs")) return -1;
			pairs.bins = atoi(argv[i + 1]);
			pairs.rmax = atof(argv[i + 2]);
			if (pairs.bins < 1 || pairs.bins > 65536 || !std::isfinite(pairs.rmax) || !(pairs.rmax > 0))
			{
				std::cerr << "Error: invalid argument(s) to '-pairs': " << argv[i + 1] << ' ' << argv[i + 2] << " (1..65536 bins, rmax greater than 0)\n";
				return -1;
			}
			i += 2;
		}
		else if (a == "-solid")
		{
			if (!need(i, 3, "-solid")) return -1;
			solid.rmax = atof(argv[i + 1]);
			solid.dmin = atof(argv[i + 2]);
			char *end = nullptr;
			const long xm = strtol(argv[i + 3], &end, 10);
			if (!std::isfinite(solid.rmax) || !(solid.rmax > 0) || !std::isfinite(solid.dmin) || end == argv[i + 3] || *end || xm < 0 || xm > 0x7fffffffL)
			{
				std::cerr << "Error: invalid argument to '-solid': " << argv[i + 1] << ' ' << argv[i + 2] << ' ' << argv[i + 3]
				          << " (rmax greater than 0, dmin finite, xi_min a non-negative integer)\n";
				return -1;
			}
			solid.xi_min = (int)xm;
			i += 3;
		}
		else if (a == "-bonds")
		{
			if (!need(i, 1, "-bonds")) return -1;
			bonds_rmax = atof(argv[i + 1]);
			if (!std::isfinite(bonds_rmax) || !(bonds_rmax > 0))
			{
				std::cerr << "Error: invalid argument to '-bonds': " << argv[i + 1] << " (rmax greater than 0)\n";
				return -1;
			}
			++i;
		}
		else if (a == "-sk")
		{
			if (!need(i, 6, "-sk")) return -1;
			if (!parse_sk(3, argv + i + 1, sk))
			{
				std::cerr << "Error: invalid argument(s) to '-sk' (hx hy hz: integers 0..64; kx ky kz: finite and greater than 0)\n";
				return -1;
			}
			i += 6;
		}
		else if (a == "-corr")
		{
			if (!need(i, 3, "-corr")) return -1;
			if (!parse_corr(argv + i + 1, corr))
			{
				std::cerr << "Error: invalid argument(s) to '-corr' (stride: an integer >= 1; frames, lags: integers with 1 <= lags <= frames <= 2048)\n";
				return -1;
			}
			i += 3;
		}
		else if (a == "-corr-start")
		{
			if (!need(i, 1, "-corr-start")) return -1;
			char *end = nullptr;
			const long v = std::strtol(argv[i + 1], &end, 10);
			if (end == argv[i + 1] || *end || v < 0 || v > 0x7fffffffL) { std::cerr << "Error: invalid argument to '-corr-start': " << argv[i + 1] << " (an iteration >= 0)\n"; return -1; }
			corr.start = (int)v;
			++i;
		}
		else if (a == "-modes")
		{
			if (!need(i, 8, "-modes")) return -1;
			if (!parse_modes(argv + i + 1, modes))
			{
				std::cerr << "Error: invalid argument(s) to '-modes' (hx hy hz: integers 0..64; kx ky kz: finite and greater than 0; frames, lags: integers with 1 <= lags <= frames <= 1024)\n";
				return -1;
			}
			i += 8;
		}
		else if (a == "-modes-start")
		{
			if (!need(i, 1, "-modes-start")) return -1;
			char *end = nullptr;
			const long v = std::strtol(argv[i + 1], &end, 10);
			if (end == argv[i + 1] || *end || v < 0 || v > 0x7fffffffL) { std::cerr << "Error: invalid argument to '-modes-start': " << argv[i + 1] << " (an iteration >= 0)\n"; return -1; }
			modes.start = (int)v;
			++i;
		}
		else if (a == "-aperture")
		{
			if (!need(i, 4, "-aperture")) return -1;
			const std::string_view v(argv[i + 1]);
			bool ok = v == "ellipsoid" || v == "box";
			aperture.ap.shape = v == "box" ? NBCO_AP_BOX : NBCO_AP_ELLIPSOID;
			for (int k = 0; k < 3; ++k)
			{
				aperture.ap.half[k] = atof(argv[i + 2 + k]);   // ('inf' opens the axis)
				ok = ok && aperture.ap.half[k] > 0;
			}
			if (!ok)
			{
				std::cerr << "Error: invalid argument(s) to '-aperture': " << argv[i + 1] << ' ' << argv[i + 2] << ' ' << argv[i + 3] << ' ' << argv[i + 4]
				          << " (ellipsoid or box, three half axes greater than 0)\n";
				return -1;
			}
			aperture.on = true;
			i += 4;
		}
		else if (a == "-aperture-centre")
		{
			if (!need(i, 3, "-aperture-centre")) return -1;
			for (int k = 0; k < 3; ++k) aperture.ap.centre[k] = atof(argv[i + 1 + k]);
			if (!std::isfinite(aperture.ap.centre[0]) || !std::isfinite(aperture.ap.centre[1]) || !std::isfinite(aperture.ap.centre[2]))
			{
				std::cerr << "Error: invalid argument(s) to '-aperture-centre': " << argv[i + 1] << ' ' << argv[i + 2] << ' ' << argv[i + 3] << '\n';
				return -1;
			}
			i += 3;
		}
		else if (a == "-B")
		{
			if (!need(i, 3, "-B")) return -1;
			for (int k = 0; k < 3; ++k) omega_b[k] = atof(argv[i + 1 + k]);
			if (!std::isfinite(omega_b[0]) || !std::isfinite(omega_b[1]) || !std::isfinite(omega_b[2]))
			{
				std::cerr << "Error: invalid argument(s) to '-B': " << argv[i + 1] << ' ' << argv[i + 2] << ' ' << argv[i + 3] << " (three finite components)\n";
				return -1;
			}
			bfield = omega_b[0] != 0 || omega_b[1] != 0 || omega_b[2] != 0;   // (0 0 0 IS the run without the flag, on the host path too)
			i += 3;
		}
		else if (a == "-bath")
		{
			if (!need(i, 6, "-bath")) return -1;
			bool ok = true;
			for (int k = 0; k < 3; ++k)
			{
				bath.gamma[k] = atof(argv[i + 1 + k]);
				bath.kT[k] = atof(argv[i + 4 + k]);
				ok = ok && std::isfinite(bath.gamma[k]) && bath.gamma[k] >= 0 && std::isfinite(bath.kT[k]) && bath.kT[k] >= 0;
			}
			if (!ok)
			{
				std::cerr << "Error: invalid argument(s) to '-bath' (three rates and three temperatures, finite and not negative)\n";
				return -1;
			}
			bath_on = bath.gamma[0] != 0 || bath.gamma[1] != 0 || bath.gamma[2] != 0;   // (all rates 0 IS the run without the flag, on the host path too)
			i += 6;
		}
		else if (a == "-bath-seed")
		{
			if (!need(i, 1, "-bath-seed")) return -1;
			char *end = nullptr;
			bath.seed = strtoull(argv[i + 1], &end, 10);
			if (end == argv[i + 1] || *end != 0 || argv[i + 1][0] == '-') { std::cerr << "Error: invalid argument to '-bath-seed': " << argv[i + 1] << " (an unsigned 64-bit integer)\n"; return -1; }
			i += 1;
		}
		else if (a == "-cpu-threads")
		{
			if (!need(i, 1, "-cpu-threads")) return -1;
			nbco_cpu::threads() = atoi(argv[i + 1]);
			if (nbco_cpu::threads() <= 0) { std::cerr << "Error: invalid argument to '-cpu-threads': " << argv[i + 1] << " (should be greater than 0)\n"; return -1; }
			++i;
		}
		else if (a == "-cacheline")
		{
			if (!need(i, 1, "-cacheline")) return -1;   // (main3.cu: cache-line padding of the reference's CPU FMM; nothing to tune here)
			++i;
		}
		else if (a == "-snapshot-order")
		{
			if (!need(i, 1, "-snapshot-order")) return -1;
			const std::string_view v(argv[i + 1]);
			if (v == "input") input_order = true;
			else if (v == "tree") input_order = false;
			else { std::cerr << "Error: invalid argument to '-snapshot-order': " << argv[i + 1] << '\n'; return -1; }
			++i;
		}
		else if (a == "-test") test = true;
		else if (a == "-test2") test2 = true;
		else if (a == "-xi")
		{
			if (!need(i, 1, "-xi")) return -1;
			xi = (SCAL)atof(argv[i + 1]);
			if (xi < 0) { std::cerr << "Error: invalid argument to '-xi': " << argv[i + 1] << '\n'; return -1; }
			++i;
		}
		else if (a == "-omega0")
		{
			if (!need(i, 2, "-omega0")) return -1;
			omega0.x = (SCAL)atof(argv[i + 1]); omega0.y = (SCAL)atof(argv[i + 2]);   // main3.cu:568-569 (z is not read)
			if (omega0.x < 0 || omega0.y < 0) { std::cerr << "Error: invalid argument(s) to '-omega0': " << argv[i + 1] << ' ' << argv[i + 2] << '\n'; return -1; }
			i += 2;
		}
		else if (a == "-x" || a == "-u")
		{
			if (!need(i, 3, a == "-x" ? "-x" : "-u")) return -1;
			V3 v{(SCAL)atof(argv[i + 1]), (SCAL)atof(argv[i + 2]), (SCAL)atof(argv[i + 3])};
			if (v.x < 0 || v.y < 0 || v.z < 0) { std::cerr << "Error: invalid argument(s) to '" << a << "': " << argv[i + 1] << ' ' << argv[i + 2] << ' ' << argv[i + 3] << '\n'; return -1; }
			(a == "-x" ? x : u) = v;
			i += 3;
		}
		else { std::cerr << "Error: unrecognised option '" << argv[i] << "'\n"; return -1; }
	}

	if (aperture.on && (test || test2 || b_accuracy))
	{
		std::cerr << "Error: '-aperture' changes the run: it cannot be combined with -test, -test2 or -accuracy\n";
		return -1;
	}

	if (corr.on && (test || test2 || b_accuracy))
	{
		std::cerr << "Error: '-corr' follows a simulation: it cannot be combined with -test, -test2 or -accuracy\n";
		return -1;
	}

	if (modes.on && (test || test2 || b_accuracy))
	{
		std::cerr << "Error: '-modes' follows a simulation: it cannot be combined with -test, -test2 or -accuracy\n";
		return -1;
	}

	// ---- state ---------------------------------------------------------------------------------------
	std::vector<float> host;   // [pos | vel] as the state files hold them; the accelerations never leave the device
	if (in)
	{
		std::ifstream fin(strin, std::ios::in | std::ios::binary | std::ios::ate);
		if (!fin) { std::cerr << "Error: cannot read from input location." << std::endl; return -1; }
		const std::streamoff len = fin.tellg();
		nBodies = (int)((size_t)len / 2 / sizeof(V3));       // main3.cu:636
		host.resize(6 * (size_t)nBodies);
		fin.seekg(0, std::ios::beg);
		fin.read(reinterpret_cast<char *>(host.data()), (std::streamsize)(host.size() * sizeof(float)));
	}
	else
	{
		host.resize(6 * (size_t)nBodies);
		const float sx[3]{x.x, x.y, x.z}, su[3]{u.x, u.y, u.z};
		// main3.cu:662-666: mt19937_64(5351550349027530206), discard(624 * 2), initGA, and initU over the same stream for -test
		if (nbco_init_gaussian(host.data(), nBodies, sx, su, NBCO_REF_SEED, NBCO_REF_DISCARD, test ? 1 : 0) != NBCO_OK)
		{
			std::cerr << "Error: cannot sample the initial state." << std::endl;
			return -1;
		}
	}
	if (nBodies <= 0) { std::cerr << "Error: no particles." << std::endl; return -1; }
	size_t state_bytes = host.size() * sizeof(float);

	if (!test && !test2)
	{
		std::ofstream farg(strout + "/args.txt", std::ios::out);   // main3.cu:669-683
		if (!farg)
		{
			std::cerr << "Error: cannot write on output location. Check that \"" << strout << "\" folder exists. Create it if not." << std::endl;
			return -1;
		}
		for (int i = 0; i < argc; ++i) farg << argv[i] << ' ';
	}

	const SCAL par[6]{xi / (SCAL)nBodies, 0, 0, omega0.x * omega0.x, omega0.y * omega0.y, omega0.z * omega0.z};   // main3.cu:685-692

	if (cpu)
	{
		// BASELINE config 1: the same loop and files with the host evaluator (coulombOscillatorDirect_cpu, main3.cu:53-57, :844)
		if (test || test2 || b_accuracy) { std::cerr << "Error: '-cpu' runs the simulation only: -test, -test2 and -accuracy need the GPU\n"; return -1; }
		if (input_order) { std::cerr << "Error: '-snapshot-order input' is what '-cpu' writes anyway (the direct sum never permutes the state)\n"; return -1; }
		std::vector<nbco_cpu::V3> st(3 * (size_t)nBodies);
		std::memcpy(st.data(), host.data(), state_bytes);
		nbco_cpu::force(st.data(), nBodies, par, o.eps2);
		EnergyLog elog(energy, strout);
		MomentsLog mlog(moments, strout);
		std::vector<double> probes_out(4 * (probes.size() / 3));
		std::vector<unsigned long long> pairs_counts;
		std::vector<double> pairs_nn2(pairs.bins ? (size_t)nBodies : 0);
		std::vector<int> bonds_nb;
		std::vector<double> bonds_q;
		BondsLog blog(bonds_rmax, strout);
		std::vector<int> solid_nb, solid_xi;
		std::vector<double> solid_q;
		SolidLog slog(solid, strout);
		std::vector<double> sk_rho;
		SkLog sklog(3, sk, strout);
		LossLog llog(aperture.on, strout);
		std::vector<int> lost_rows;
		std::vector<float> lost_recs;
		std::vector<nbco_moments> slice_recs;
		// -corr: the window of frames on the host, and the particle numbers of the state rows (the direct sum never permutes; an
		// aperture compacts them with the state)
		CorrWindow cwin(corr, nBodies);
		std::vector<float> corr_traj(corr.on ? (size_t)cwin.rows * (size_t)corr.frames * 6 : 0);
		std::vector<int> corr_ids(corr.on ? (size_t)nBodies : 0);
		for (size_t i = 0; i < corr_ids.size(); ++i) corr_ids[i] = (int)i;
		auto corr_finish = [&]() {
			std::vector<nbco_corr_lag> rec;
			if (cwin.lags() > 0) nbco_cpu::time_corr(corr_traj.data(), cwin.rows, corr.frames, cwin.recorded, cwin.lags(), rec);
			if (cwin.write(strout, rec, (double)nSteps * (double)dt)) return true;
			std::cerr << "Error: cannot write the correlation files into \"" << strout << "\"" << std::endl;
			return false;
		};
		// -modes: the series of mode records on the host
		ModesWindow mwin(modes);
		std::vector<double> modes_series(modes.on ? (size_t)modes.K * (size_t)modes.frames * 8 : 0);
		auto modes_finish = [&]() {
			std::vector<nbco_mode_lag> rec((size_t)modes.K * (size_t)mwin.lags());
			std::vector<double> rho0;
			if (!rec.empty())
			{
				if (nbco_mode_corr_ref(modes_series.data(), &modes.g, modes.frames, mwin.recorded, mwin.lags(), rec.data()) != NBCO_OK)
				{
					std::cerr << "Error: nbco_mode_corr_ref refused the recorded series" << std::endl;
					return false;
				}
				for (int f = 0; f < mwin.recorded; ++f) rho0.push_back(modes_series[(mwin.k0() * (size_t)modes.frames + (size_t)f) * 8]);
			}
			if (mwin.write(strout, rec, rho0)) return true;
			std::cerr << "Error: cannot write the modes files into \"" << strout << "\"" << std::endl;
			return false;
		};
		for (int iter = 0; iter < nIters; ++iter)
		{
			nbco_cpu::integrate(scheme, st.data(), nBodies, par, o.eps2, (long double)dt, bfield ? omega_b : nullptr, bath_on ? &bath : nullptr, (unsigned long long)iter);
			if (iter % nSteps != 0) continue;
			std::cout << iter << ' ' << std::flush;
			if (aperture.on)
			{
				// (the direct sum never permutes the state: a row is a particle number until somebody is lost)
				nbco_cpu::aperture_apply(st, nBodies, aperture.ap.shape, aperture.ap.centre, aperture.ap.half, lost_rows, lost_recs);
				if (corr.on && !lost_rows.empty())
				{
					size_t next = 0, w = 0;
					for (size_t i = 0; i < corr_ids.size(); ++i)
					{
						if (next < lost_rows.size() && (size_t)lost_rows[next] == i) ++next;
						else corr_ids[w++] = corr_ids[i];
					}
					corr_ids.resize(w);
				}
				state_bytes = 6 * (size_t)nBodies * sizeof(float);
				pairs_nn2.resize(pairs.bins ? (size_t)nBodies : 0);
				if (!llog.record(iter, dt, lost_rows, lost_recs, nBodies)) return -1;
				if (nBodies == 0)
				{
					std::cerr << "\nError: every particle is outside the aperture at iteration " << iter << ": nothing is left to simulate" << std::endl;
					return -1;
				}
			}
			if (const int frame = cwin.frame_for(iter); frame >= 0)
			{
				nbco_cpu::traj_record(st.data(), nBodies, corr_ids, corr_traj, cwin.rows, corr.frames, frame, corr.stride);
				++cwin.recorded;
				if (cwin.full() && !corr_finish()) return -1;
			}
			if (const int frame = mwin.frame_for(iter); frame >= 0)
			{
				nbco_cpu::modes_record(st.data(), nBodies, modes.g, modes_series, modes.frames, frame);
				++mwin.recorded;
				if (mwin.full() && !modes_finish()) return -1;
			}
			std::ofstream fout(strout + "/out" + std::to_string(iter) + '_' + std::to_string(dt) + ".bin", std::ios::out | std::ios::binary);
			if (!fout)
			{
				std::cerr << "Error: cannot write on output location. Check that \"" << strout << "\" folder exists. Create it if not." << std::endl;
				return -1;
			}
			fout.write(reinterpret_cast<const char *>(st.data()), (std::streamsize)state_bytes);
			if (energy)
			{
				double e3[3];
				nbco_cpu::energy(st.data(), nBodies, par, o.eps2, e3);
				elog.line(iter, e3);
			}
			if (moments)
			{
				nbco_moments mom{};
				mom.n = nBodies;
				mom.dim = 3;
				nbco_cpu::moment_sums(st.data(), nBodies, mom.mean, mom.min, mom.max, mom.cov, mom.m4);
				nbco_moments_derive(&mom);
				mlog.line(iter, mom);
			}
			if (slices.on)
			{
				const long long outside = nbco_cpu::slice_moments(st.data(), nBodies, slices.axis, slice_recs);
				if (!write_slices(strout, iter, std::to_string(dt), 3, slices.axis, slice_recs.data(), outside))
				{
					std::cerr << "Error: cannot write the slice file of iteration " << iter << " into \"" << strout << "\"" << std::endl;
					return -1;
				}
			}
			if (!probes.empty())
			{
				cpu_probes(st.data(), nBodies, probes, par, o.eps2, probes_out);
				if (!write_probes(strout, iter, dt, probes_out)) return -1;
			}
			if (pairs.bins)
			{
				nbco_cpu::pair_stats(st.data(), nBodies, pairs.bins, pairs.rmax, pairs_counts, pairs_nn2);
				if (!write_pairs(strout, iter, dt, pairs_counts, pairs_nn2)) return -1;
			}
			if (bonds_rmax > 0)
			{
				nbco_bond_summary bsum;
				nbco_cpu::bond_order(st.data(), nBodies, bonds_rmax, bonds_nb, bonds_q, bsum);
				if (!blog.record(iter, dt, bonds_nb, bonds_q, bsum)) return -1;
			}
			if (solid.rmax > 0)
			{
				nbco_solid_summary ssum;
				nbco_cpu::bond_solid(st.data(), nBodies, solid.rmax, solid.dmin, solid.xi_min, solid_nb, solid_xi, solid_q, ssum);
				if (!slog.record(iter, dt, solid_nb, solid_xi, solid_q, ssum)) return -1;
			}
			if (sk.on)
			{
				const long long n_used = nbco_cpu::structure_factor(st.data(), nBodies, sk.g, sk_rho);
				if (!sklog.record(iter, std::to_string(dt), sk_rho, n_used))
				{
					std::cerr << "Error: cannot write the structure factor files of iteration " << iter << " into \"" << strout << "\"" << std::endl;
					return -1;
				}
			}
		}
		if (corr.on && !cwin.written && !corr_finish()) return -1;
		if (modes.on && !mwin.written && !modes_finish()) return -1;
		std::cout << std::endl;
		return 0;
	}

	Session s(o, nBodies, host, par);
	int rc = 0;
	if (b_accuracy) rc = s.search_parameters(accuracy);
	if (rc == 0)
	{
		if (test) s.print_error_table(host);
		else if (test2) s.print_reuse_errors(dt);
		else rc = s.simulate(scheme, dt, nIters, nSteps, strout, host, state_bytes, input_order, energy && !b_accuracy, moments && !b_accuracy, b_accuracy ? std::vector<float>{} : probes,
		                     b_accuracy ? PairsOpt{} : pairs, b_accuracy ? 0.0 : bonds_rmax, b_accuracy ? SolidOpt{} : solid, b_accuracy ? SkOpt{} : sk, aperture, b_accuracy ? SlicesOpt{} : slices, bfield && !b_accuracy ? omega_b : nullptr,
		                     b_accuracy ? nbco_bath{} : bath, corr, modes);
	}
	return rc;
}
