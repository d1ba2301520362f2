// nbco -- the reference's 2-D program (Simulation/main.cu: N charges in a 2-D anisotropic trap, fp64, a KV beam by default) over
// the C ABI of libnbco_hip.so.  Flags, defaults, exit codes, error strings, the initial state, args.txt and the snapshot files
// follow main.cu:257-903; the evaluator is nbco_2d_fmm (fmm_cart) plus the elastic term, integrated by nbco_2d_integrate.
//
// Additions: -energy writes the energies of every snapshot to energy.txt (nbco_2d_energy_fmm); -probes <file> writes the field and
// the potential at the file's points for every snapshot (nbco_2d_probe_fmm); -moments writes the beam's phase-space moments of every
// snapshot to moments.txt (nbco_2d_beam_moments); -slices writes them per slice along one coordinate to slices<iter>_<ds>.txt
// (nbco_2d_slice_moments); -sk writes the static structure factor of every snapshot to sk<iter>_<ds>.bin and sk.txt
// (nbco_2d_structure_factor); without them nothing changes.
// Deviations: -cpu / -cpu-threads are refused (main.cu -cpu runs a host FMM, which this product does not have); -gpu, -gridsize
// and -cacheline are validated as main.cu does and then have no effect; -p above 10 is refused by the library (NBCO_ERR_ARG).
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <vector>
#include "../../include/nbco.h"
#include "slices_file.hpp"
#include "sk_file.hpp"

namespace {

struct V2 { double x, y; };

const char *kHelp =
    "nbco: 2-D Coulomb oscillators (fp64 quadtree FMM on an AMD Instinct GPU).\n\n"
    "Usage: nbco [options] [input]\n\n"
    "  input             binary state file: all positions, then all velocities, as pairs of doubles\n"
    "                    (N = file size / 32).  Without it the state is drawn from a KV distribution\n"
    "                    (or a Gaussian one with -ga).\n\n"
    "Options:\n"
    "  -h, -help         print this text\n"
    "  -o <dir>          existing folder for args.txt and the snapshots (default ./out); each snapshot\n"
    "                    out<iter>_<ds>.bin holds positions and velocities in the input file's format,\n"
    "                    in the tree order of the evaluation\n"
    "  -n <N>            particle count without an input file (default 30001)\n"
    "  -ds <v>           time step (default 5e-4)\n"
    "  -iters <k>        the run takes k + 1 steps (default 30000)\n"
    "  -steps <k>        a snapshot every k steps (default 200)\n"
    "  -integ <name>     integrator instead of leapfrog; the name follows one leading character, as in\n"
    "                    the original parser: -eu (symplectic Euler), -fr (Forest-Ruth), -pefrl (PEFRL)\n"
    "  -p <order>        expansion order, 1..10 (default 5)\n"
    "  -r <radius>       near-field radius in leaf cells, integer >= 1 (default 1)\n"
    "  -eps <v>          softening length, > 0 (default 1e-9; EPS2 = v^2)\n"
    "  -i <v>            density factor of the level count round(log4(N v / p^1.5)) (default 1)\n"
    "  -ncoll            skip the near field (a is scaled by 0 there instead)\n"
    "  -test             time one evaluation, then print the mean relative error against the\n"
    "                    compensated direct sum for p = 1..10; no snapshots\n"
    "  -energy           at every snapshot append `iter kinetic elastic coulomb total` to <dir>/energy.txt:\n"
    "                    the O(N) FMM potential energy of the snapshot's state (nbco_2d_energy_fmm, order -p);\n"
    "                    no effect with -test\n"
    "  -moments          at every snapshot append the beam's phase-space moments to <dir>/moments.txt\n"
    "                    (nbco_2d_beam_moments): `iter`, the means of (x, y, vx, vy), then per plane (x, vx), (y, vy)\n"
    "                    `sig_q sig_p cov_qp emit halo_q halo`; the file starts with a `#` line naming the columns;\n"
    "                    no effect with -test\n"
    "  -slices <x|y|vx|vy> <bins> <lo> <hi>\n"
    "                    at every snapshot write the moments of -moments per slice along that coordinate to\n"
    "                    <dir>/slices<iter>_<ds>.txt (nbco_2d_slice_moments): a particle's slice is the bin\n"
    "                    (int) ((q - lo) bins / (hi - lo)) of the window lo <= q < hi; a `#` line names the columns,\n"
    "                    `# outside <k>` counts the particles outside the window, then one line per slice: `s lo_s n`,\n"
    "                    the 4 means, then per plane `sig_q sig_p cov_qp emit halo_q halo` of the slice's particles\n"
    "                    alone (an empty slice: zeros); no effect with -test\n"
    "  -sk <hx> <hy> <kx> <ky>\n"
    "                    at every snapshot write the static structure factor of the positions to <dir>/sk<iter>_<ds>.bin\n"
    "                    (nbco_2d_structure_factor): K x 2 doubles {re, im} of rho_k = sum_j exp(i k . x_j), k = (ix kx, iy ky),\n"
    "                    ix = 0..hx, iy = -hy..hy (h <= 64), K = (hx+1)(2hy+1), index ix (2hy+1) + iy + hy; and append\n"
    "                    `iter n_used S_max ix iy` to <dir>/sk.txt: the largest |rho_k|^2 / n_used over k != 0\n"
    "  -probes <file>    binary file of probe points as pairs of doubles (M = file size / 16).  At every snapshot\n"
    "                    write <dir>/probes<iter>_<ds>.bin: the M accelerations (pairs) and then the M potentials\n"
    "                    of the snapshot's particles at these points (nbco_2d_probe_fmm, order -p; the points feel\n"
    "                    the beam and do not act on it); no effect with -test\n"
    "  -aperture <ellipse|box> <hx> <hy>\n"
    "                    at every snapshot iteration, after the step and before the snapshot, drop the particles outside\n"
    "                    the aperture with these half axes about the origin (`inf` opens an axis) from the run\n"
    "                    (nbco_2d_aperture_apply): <dir>/lost<iter>_<ds>.bin receives k int32 rows (the rows the lost\n"
    "                    particles had in the state), then k x 4 doubles x y vx vy -- empty when nobody was lost -- and\n"
    "                    <dir>/losses.txt one line `iter n_lost n_left`; the snapshot and -energy, -moments, -probes\n"
    "                    describe the survivors, and the snapshot files shrink with n; a run that loses everybody ends\n"
    "                    with an error; refused with -test\n"
    "  -B <w>            uniform magnetic field out of the plane, Omega = (q/m) B in radians per unit of -ds: the force\n"
    "                    (vy, -vx) w, integrated exactly -- the drift of every scheme becomes a rotation\n"
    "                    (nbco_2d_integrate_b); 0 is the run without the flag; no effect with -test\n"
    "  -bath <gx> <gy> <Tx> <Ty>   Langevin bath: friction rates per unit of -ds and temperatures (units of v^2) per\n"
    "                    axis; every step is wrapped in two exact half steps of friction and noise\n"
    "                    (nbco_2d_integrate_t), the iteration number is the tick; rates 0 0 are the run without the\n"
    "                    flag; -bath-seed <u64> seeds the noise; works with -B; no effect with -test\n"
    "  -ga               Gaussian initial state instead of KV\n"
    "  -xi <v>           perveance\n"
    "  -omega0 <x> <y>   trap phase advances\n"
    "  -x <x> <y>        position spread (sets A = 2 x)\n"
    "  -u <x> <y>        velocity spread (omega follows as u / x)\n"
    "  -A <x> <y>        semi-axes (sets x = A / 2)\n"
    "  -omega <x> <y>    depressed phase advances (u follows as omega x)\n"
    "  -gpu <n>, -gridsize <n>, -cacheline <n>\n"
    "                    accepted for compatibility (n >= 1); no effect\n"
    "  -cpu, -cpu-threads <n>\n"
    "                    not available: this build has no host evaluator\n";

int fail(const std::string &msg)
{
	std::cerr << msg;
	return -1;
}

bool is(const char *a, const char *name) { return std::strcmp(a + 1, name) == 0; }

}  // namespace

int main(const int argc, const char **argv)
{
	int nBodies = 30001, nIters = 30001, nSteps = 200, integ = NBCO_INTEG_LEAPFROG;
	int fmm_order = 5, tree_radius = 1;
	double dt = 5.e-4, EPS2 = 1e-18, dens_inhom = 1, omega_b = 0;
	nbco_bath bath{{0, 0, 0}, {0, 0, 0}, NBCO_REF_SEED};
	std::string strout("out"), strin, strprobes;
	bool in = false, cpu = false, test = false, ga = false, calc_u = false, calc_omega = false, coll = true, energy = false, moments = false;
	bool aperture = false;
	SlicesOpt slices;
	SkOpt sk;
	nbco_aperture ap{NBCO_AP_ELLIPSOID, {0, 0, 0}, {0, 0, 0}};

	// KV parameters matched to the emittances (main.cu:271-313)
	const double twopi = 6.283185307179586476925286766559;
	double xi = 2.e-6;
	V2 omega0{6.22 * twopi, 6.21 * twopi};
	V2 emit{0.03e-3, 0.01e-3}, omega, domega, A, x, u;
	omega.y = 0.8 * omega0.y;
	A.y = 2 * std::sqrt(emit.y / omega.y);
	const double A2 = A.y * A.y;
	domega.y = (omega0.y + omega.y) * (omega0.y - omega.y);
	const double om0x2 = omega0.x * omega0.x, om0x4 = om0x2 * om0x2, om0x6 = om0x4 * om0x2;
	const double c = -2 * om0x2, d = -A2 * domega.y * domega.y / (4 * emit.x), p = c, q = d;
	const double Delta0 = 16 * om0x4, Delta1 = 27 * d * d + 128 * om0x6;
	const double Q = std::cbrt((Delta1 + std::sqrt((27 * d * d + 256 * om0x6) * (27 * d * d))) / 2);
	const double S = std::sqrt((-2 * p + (Q + Delta0 / Q)) / 3) / 2;
	omega.x = S - std::sqrt(-4 * S * S - 2 * p - q / S) / 2;   // the quartic's fourth root
	A.x = 2 * std::sqrt(emit.x / omega.x);
	xi = domega.y * A.y * (A.x + A.y) / 2;
	x = V2{A.x / 2, A.y / 2};
	u = V2{omega.x * A.x / 2, omega.y * A.y / 2};

	auto need = [&](int i, int k, const char *) { return i + k < argc ? 0 : 1; };
	for (int i = 1; i < argc; ++i)
	{
		const char *a = argv[i];
		if (a[0] != '-') { strin = a; in = true; continue; }
		const std::string opt = std::string("'") + a + "'";
		auto missing = [&]() { return fail("Error: missing argument to " + opt + "\n"); };
		auto missing2 = [&]() { return fail("Error: missing argument(s) to " + opt + "\n"); };
		auto invalid = [&](const char *v, const char *tail = "") { return fail("Error: invalid argument to " + opt + ": " + v + tail + "\n"); };
		auto invalid2 = [&]() { return fail("Error: invalid argument(s) to " + opt + ": " + argv[i + 1] + " " + argv[i + 2] + "\n"); };
		auto int_arg = [&](int &dst) -> int {
			if (need(i, 1, a)) return missing();
			dst = std::atoi(argv[i + 1]);
			if (dst <= 0) return invalid(argv[i + 1]);
			++i;
			return 0;
		};
		auto pair_arg = [&](V2 &dst) -> int {
			if (need(i, 2, a)) return missing2();
			dst = V2{std::atof(argv[i + 1]), std::atof(argv[i + 2])};
			if (dst.x < 0 || dst.y < 0) return invalid2();
			i += 2;
			return 0;
		};
		int rc = 0, dummy = 0;
		if (is(a, "h") || is(a, "help")) { std::cout << kHelp; return 0; }
		else if (is(a, "o")) { if (need(i, 1, a)) return missing(); strout = argv[++i]; }
		else if (is(a, "n")) rc = int_arg(nBodies);
		else if (is(a, "ds"))
		{
			if (need(i, 1, a)) return missing();
			dt = std::atof(argv[i + 1]);
			if (dt <= 0) return invalid(argv[i + 1]);
			++i;
		}
		else if (is(a, "iters"))
		{
			if (need(i, 1, a)) return missing();
			nIters = std::atoi(argv[i + 1]) + 1;
			if (nIters <= 0) return invalid(argv[i + 1]);
			++i;
		}
		else if (is(a, "steps")) rc = int_arg(nSteps);
		else if (is(a, "integ"))
		{
			if (need(i, 1, a)) return missing();
			const char *v = argv[i + 1];
			// main.cu:460-476 compares the name from its second character on
			if (v[0] && is(v, "eu")) integ = NBCO_INTEG_EULER;
			else if (v[0] && is(v, "fr")) integ = NBCO_INTEG_FORESTRUTH;
			else if (v[0] && is(v, "pefrl")) integ = NBCO_INTEG_PEFRL;
			else return invalid(v);
			++i;
		}
		else if (is(a, "p")) rc = int_arg(fmm_order);
		else if (is(a, "r")) rc = int_arg(tree_radius);
		else if (is(a, "eps"))
		{
			if (need(i, 1, a)) return missing();
			EPS2 = std::atof(argv[i + 1]);
			if (EPS2 <= 0) return invalid(argv[i + 1]);
			EPS2 *= EPS2;
			if (EPS2 == 0) return fail("Error: too small argument to " + opt + ": " + argv[i + 1] + "\n");
			++i;
		}
		else if (is(a, "i"))
		{
			if (need(i, 1, a)) return missing();
			dens_inhom = std::atof(argv[i + 1]);
			if (dens_inhom <= 0) return invalid(argv[i + 1], " (should be greater than 0)");
			++i;
		}
		else if (is(a, "B"))
		{
			if (need(i, 1, a)) return missing();
			omega_b = std::atof(argv[i + 1]);
			if (!std::isfinite(omega_b)) return invalid(argv[i + 1], " (should be finite)");
			++i;
		}
		else if (is(a, "bath"))
		{
			if (need(i, 4, a)) return missing();
			for (int k = 0; k < 2; ++k)
			{
				bath.gamma[k] = std::atof(argv[i + 1 + k]);
				bath.kT[k] = std::atof(argv[i + 3 + k]);
				if (!std::isfinite(bath.gamma[k]) || bath.gamma[k] < 0) return invalid(argv[i + 1 + k], " (rates should be finite and not negative)");
				if (!std::isfinite(bath.kT[k]) || bath.kT[k] < 0) return invalid(argv[i + 3 + k], " (temperatures should be finite and not negative)");
			}
			i += 4;
		}
		else if (is(a, "bath-seed"))
		{
			if (need(i, 1, a)) return missing();
			char *end = nullptr;
			bath.seed = std::strtoull(argv[i + 1], &end, 10);
			if (end == argv[i + 1] || *end != 0 || argv[i + 1][0] == '-') return invalid(argv[i + 1], " (should be an unsigned 64-bit integer)");
			++i;
		}
		else if (is(a, "ncoll")) coll = false;
		else if (is(a, "cpu")) cpu = true;
		else if (is(a, "cpu-threads")) { cpu = true; rc = int_arg(dummy); }
		else if (is(a, "cacheline") || is(a, "gpu") || is(a, "gridsize")) rc = int_arg(dummy);
		else if (is(a, "test")) test = true;
		else if (is(a, "ga")) ga = true;
		else if (is(a, "energy")) energy = true;
		else if (is(a, "moments")) moments = true;
		else if (is(a, "slices"))
		{
			if (need(i, 4, a)) return missing2();
			if (!parse_slices(2, argv[i + 1], argv[i + 2], argv[i + 3], argv[i + 4], slices))
				return fail("Error: invalid argument(s) to " + opt + ": " + argv[i + 1] + " " + argv[i + 2] + " " + argv[i + 3] + " " + argv[i + 4] +
				            " (x, y, vx or vy, 1..65536 bins, lo below hi, both finite)\n");
			i += 4;
		}
		else if (is(a, "sk"))
		{
			if (need(i, 4, a)) return missing2();
			if (!parse_sk(2, argv + i + 1, sk)) return fail("Error: invalid argument(s) to " + opt + " (hx hy: integers 0..64; kx ky: finite and greater than 0)\n");
			i += 4;
		}
		else if (is(a, "probes")) { if (need(i, 1, a)) return missing(); strprobes = argv[++i]; }
		else if (is(a, "aperture"))
		{
			if (need(i, 3, a)) return missing2();
			const bool box = std::strcmp(argv[i + 1], "box") == 0;
			ap.shape = box ? NBCO_AP_BOX : NBCO_AP_ELLIPSOID;
			ap.half[0] = std::atof(argv[i + 2]);   // (`inf` opens the axis)
			ap.half[1] = std::atof(argv[i + 3]);
			if ((!box && std::strcmp(argv[i + 1], "ellipse") != 0) || !(ap.half[0] > 0) || !(ap.half[1] > 0))
				return fail("Error: invalid argument(s) to " + opt + ": " + argv[i + 1] + " " + argv[i + 2] + " " + argv[i + 3] +
				            " (ellipse or box, two half axes greater than 0)\n");
			aperture = true;
			i += 3;
		}
		else if (is(a, "xi"))
		{
			if (need(i, 1, a)) return missing();
			xi = std::atof(argv[i + 1]);
			if (xi < 0) return invalid(argv[i + 1]);
			++i;
		}
		else if (is(a, "omega0")) rc = pair_arg(omega0);
		else if (is(a, "x")) { rc = pair_arg(x); A = V2{x.x * 2, x.y * 2}; }
		else if (is(a, "u")) { rc = pair_arg(u); calc_omega = true; }
		else if (is(a, "A")) { rc = pair_arg(A); x = V2{A.x / 2, A.y / 2}; }
		else if (is(a, "omega")) { rc = pair_arg(omega); calc_u = true; }
		else return fail("Error: unrecognised option '" + std::string(a) + "'\n");
		if (rc) return rc;
	}
	if (cpu) return fail("Error: '-cpu' is not available: this build evaluates on the GPU only\n");
	if (aperture && test) return fail("Error: '-aperture' changes the run: it cannot be combined with -test\n");
	if (fmm_order > 10) return fail("Error: invalid argument to '-p': " + std::to_string(fmm_order) + " (orders above 10 are not provided)\n");
	if (calc_omega) omega = V2{u.x / x.x, u.y / x.y};
	else if (calc_u) u = V2{omega.x * x.x, omega.y * x.y};

	std::vector<double> probes;
	if (!strprobes.empty())
	{
		std::ifstream fpr(strprobes, std::ios::in | std::ios::binary);
		if (!fpr) return fail("Error: cannot read the probes file.\n");
		fpr.ignore(std::numeric_limits<std::streamsize>::max());
		const long long bytes = (long long)fpr.gcount();
		if (bytes <= 0 || bytes % 16 != 0) return fail("Error: the probes file must hold pairs of doubles (a multiple of 16 bytes, at least one pair).\n");
		probes.assign((size_t)(bytes / 8), 0.0);
		fpr.clear();
		fpr.seekg(0, std::ios::beg);
		fpr.read(reinterpret_cast<char *>(probes.data()), bytes);
		if (fpr.gcount() != bytes) return fail("Error: cannot read the probes file.\n");
	}
	const long long nprobes = (long long)(probes.size() / 2);

	std::vector<double> buf;
	if (in)
	{
		std::ifstream fin(strin, std::ios::in | std::ios::binary);
		if (!fin) return fail("Error: cannot read from input location.\n");
		fin.ignore(std::numeric_limits<std::streamsize>::max());
		const long long bytes = (long long)fin.gcount();
		nBodies = (int)(bytes / 32);
		if (nBodies <= 0) return fail("Error: the input file holds no particle.\n");
		buf.assign(6 * (size_t)nBodies, 0.0);
		fin.clear();
		fin.seekg(0, std::ios::beg);
		fin.read(reinterpret_cast<char *>(buf.data()), 32LL * nBodies);
	}
	else
	{
		buf.assign(6 * (size_t)nBodies, 0.0);
		std::cout << "emittances: " << x.x * u.x << ' ' << x.y * u.y << "\nperveance: " << xi << "\ndep. phase adv.: " << omega.x << ' '
		          << omega.y << "\nsemi-axes: " << A.x << ' ' << A.y << std::endl;
		const double a2[2] = {ga ? x.x : A.x, ga ? x.y : A.y}, b2[2] = {ga ? u.x : omega.x, ga ? u.y : omega.y};
		const int rc = ga ? nbco_2d_init_gaussian(buf.data(), nBodies, a2, b2, NBCO_REF_SEED, NBCO_REF_DISCARD)
		                  : nbco_2d_init_kv(buf.data(), nBodies, a2, b2, NBCO_REF_SEED, NBCO_REF_DISCARD);
		if (rc != NBCO_OK) return fail("Error: initial state failed\n");
	}
	long long n = nBodies;   // (shrinks when -aperture loses particles)

	if (!test)
	{
		std::ofstream farg(strout + "/args.txt", std::ios::out);
		if (!farg)
			return fail("Error: cannot write on output location. Check that \"" + strout + "\" folder exists. Create it if not.\n");
		for (int i = 0; i < argc; ++i) farg << argv[i] << ' ';
	}
	const double par[4] = {xi / (double)nBodies, 0, omega0.x * omega0.x, omega0.y * omega0.y};   // main.cu:803-808

	nbco_opts o;
	nbco_opts_default(&o);
	o.fmm_order = fmm_order;
	o.tree_radius = (float)tree_radius;
	o.eps2 = (float)EPS2;
	o.coll = coll ? 1 : 0;
	o.dens_inhom = (float)dens_inhom;
	o.tree_L = 0;
	o.sync = 0;
	o.stream = nullptr;
	nbco_ctx *ctx = nullptr;
	int rc = nbco_create(&ctx, &o);
	if (rc != NBCO_OK) return fail("Error: no usable GPU context (status " + std::to_string(rc) + ")\n");
	double *d_buf = nullptr, *d_par = nullptr, *d_probes = nullptr, *d_pout = nullptr;   // d_pout: nprobes pairs, then nprobes potentials
	auto hip_ok = [&](hipError_t e) {
		if (e != hipSuccess) std::cerr << "Error: " << hipGetErrorString(e) << '\n';
		return e == hipSuccess;
	};
	auto done = [&](int code) {
		if (d_buf) (void)hipFree(d_buf);
		if (d_par) (void)hipFree(d_par);
		if (d_probes) (void)hipFree(d_probes);
		if (d_pout) (void)hipFree(d_pout);
		nbco_destroy(ctx);
		return code;
	};
	auto lib_ok = [&](int r) {
		if (r != NBCO_OK) std::cerr << "Error: " << nbco_last_error(ctx) << '\n';
		return r == NBCO_OK;
	};
	size_t cpy = sizeof(double) * 4 * (size_t)n;
	if (!hip_ok(hipMalloc(&d_buf, sizeof(double) * 6 * (size_t)n)) || !hip_ok(hipMalloc(&d_par, sizeof par)) ||
	    !hip_ok(hipMemcpy(d_buf, buf.data(), cpy, hipMemcpyHostToDevice)) || !hip_ok(hipMemcpy(d_par, par, sizeof par, hipMemcpyHostToDevice)))
		return done(-1);

	if (test)   // main.cu:823-852
	{
		if (!lib_ok(nbco_2d_force(ctx, NBCO_2D_EVAL_FMM, d_buf, n, d_par, 0)) || !lib_ok(nbco_sync(ctx))) return done(-1);
		const auto t0 = std::chrono::steady_clock::now();
		if (!lib_ok(nbco_2d_force(ctx, NBCO_2D_EVAL_FMM, d_buf, n, d_par, 0)) || !lib_ok(nbco_sync(ctx))) return done(-1);
		const auto t1 = std::chrono::steady_clock::now();
		std::cout << "Time elapsed: " << std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count() * 1.e-6 << " [s]" << std::endl;
		double *d_tmp = nullptr;
		if (!hip_ok(hipMalloc(&d_tmp, sizeof(double) * 2 * (size_t)n))) return done(-1);
		for (int order = 1; order <= 10; ++order)
		{
			o.fmm_order = order;
			double err = 0;
			if (!lib_ok(nbco_set_opts(ctx, &o)) || !lib_ok(nbco_2d_force(ctx, NBCO_2D_EVAL_FMM, d_buf, n, d_par, 0)) ||
			    !hip_ok(hipMemcpy(d_tmp, d_buf + 4 * n, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToDevice)) ||
			    !lib_ok(nbco_2d_force(ctx, NBCO_2D_EVAL_DIRECT_KAHAN, d_buf, n, d_par, 0)) ||
			    !lib_ok(nbco_2d_mean_relerr(ctx, d_tmp, d_buf + 4 * n, n, &err)))
			{
				(void)hipFree(d_tmp);
				return done(-1);
			}
			std::cout << order << ": Relative error: " << err << std::endl;
		}
		(void)hipFree(d_tmp);
		return done(0);
	}

	// main.cu:853-893: one evaluation, then per iteration a step and every nSteps iterations a snapshot
	FILE *fen = nullptr;
	if (energy && !(fen = std::fopen((strout + "/energy.txt").c_str(), "w")))
	{
		std::cerr << "Error: cannot write on output location. Check that \"" << strout << "\" folder exists. Create it if not." << std::endl;
		return done(-1);
	}
	FILE *fmo = nullptr;
	if (moments)
	{
		if (!(fmo = std::fopen((strout + "/moments.txt").c_str(), "w")))
		{
			std::cerr << "Error: cannot write on output location. Check that \"" << strout << "\" folder exists. Create it if not." << std::endl;
			if (fen) std::fclose(fen);
			return done(-1);
		}
		std::fprintf(fmo, "# iter mean_x mean_y mean_vx mean_vy");
		for (const char *k : {"x", "y"}) std::fprintf(fmo, " sig_%s sig_v%s cov_%s_v%s emit_%s halo_q_%s halo_%s", k, k, k, k, k, k, k);
		std::fprintf(fmo, "\n");
		std::fflush(fmo);
	}
	std::vector<nbco_moments> slice_recs(slices.on ? (size_t)slices.axis.bins : 0);
	// -sk: rho on the device, its host copy and <dir>/sk.txt
	double *d_rho = nullptr;
	std::vector<double> rho_host(sk.on ? 2 * (size_t)sk.K : 0);
	SkLog sklog(2, sk, strout);
	std::vector<double> pout;
	if (nprobes > 0)
	{
		pout.assign(3 * (size_t)nprobes, 0.0);
		if (!hip_ok(hipMalloc(&d_probes, sizeof(double) * 2 * (size_t)nprobes)) || !hip_ok(hipMalloc(&d_pout, sizeof(double) * 3 * (size_t)nprobes)) ||
		    !hip_ok(hipMemcpy(d_probes, probes.data(), sizeof(double) * 2 * (size_t)nprobes, hipMemcpyHostToDevice)))
		{
			if (fen) std::fclose(fen);
			if (fmo) std::fclose(fmo);
			return done(-1);
		}
	}
	// -aperture: the loss record on the device (room for everybody), its host copies and <dir>/losses.txt
	double *d_lost = nullptr;
	int *d_lost_row = nullptr;
	FILE *flo = nullptr;
	std::vector<double> lost_recs;
	std::vector<int> lost_rows;
	auto finish = [&](int code) {
		if (fen) std::fclose(fen);
		if (fmo) std::fclose(fmo);
		if (flo) std::fclose(flo);
		if (d_lost) (void)hipFree(d_lost);
		if (d_lost_row) (void)hipFree(d_lost_row);
		if (d_rho) (void)hipFree(d_rho);
		return done(code);
	};
	if (aperture)
	{
		if (!(flo = std::fopen((strout + "/losses.txt").c_str(), "w")))
		{
			std::cerr << "Error: cannot write on output location. Check that \"" << strout << "\" folder exists. Create it if not." << std::endl;
			return finish(-1);
		}
		if (!hip_ok(hipMalloc(&d_lost, sizeof(double) * 4 * (size_t)n)) || !hip_ok(hipMalloc(&d_lost_row, sizeof(int) * (size_t)n))) return finish(-1);
	}
	if (!lib_ok(nbco_2d_force(ctx, NBCO_2D_EVAL_FMM, d_buf, n, d_par, 1))) return finish(-1);
	for (int iter = 0; iter < nIters; ++iter)
	{
		if (!lib_ok(nbco_2d_integrate_t(ctx, integ, NBCO_2D_EVAL_FMM, d_buf, n, d_par, dt, 1.0, 1, omega_b, &bath, (unsigned long long)iter))) return finish(-1);
		if (iter % nSteps == 0)
		{
			std::cout << iter << ' ' << std::flush;
			if (aperture)
			{
				// the lost particles leave the state on the device: [pos n | vel n | acc n] -> [pos n' | vel n' | acc n'], order kept
				long long kept = 0;
				if (!lib_ok(nbco_2d_aperture_apply(ctx, d_buf, n, &ap, &kept, d_lost, d_lost_row, n))) return finish(-1);
				const size_t k = (size_t)(n - kept);
				lost_rows.resize(k);
				lost_recs.resize(4 * k);
				if (k && (!hip_ok(hipMemcpy(lost_rows.data(), d_lost_row, sizeof(int) * k, hipMemcpyDeviceToHost)) ||
				          !hip_ok(hipMemcpy(lost_recs.data(), d_lost, sizeof(double) * 4 * k, hipMemcpyDeviceToHost))))
					return finish(-1);
				std::ofstream flost(strout + "/lost" + std::to_string(iter) + '_' + std::to_string(dt) + ".bin", std::ios::out | std::ios::binary);
				if (flost) flost.write(reinterpret_cast<const char *>(lost_rows.data()), (std::streamsize)(sizeof(int) * k));
				if (flost) flost.write(reinterpret_cast<const char *>(lost_recs.data()), (std::streamsize)(sizeof(double) * 4 * k));
				if (!flost)
				{
					std::cerr << "Error: cannot write on output location. Check that \"" << strout << "\" folder exists. Create it if not." << std::endl;
					return finish(-1);
				}
				std::fprintf(flo, "%d %zu %lld\n", iter, k, kept);
				std::fflush(flo);
				n = kept;
				cpy = sizeof(double) * 4 * (size_t)n;
				if (n == 0)
				{
					std::cerr << "\nError: every particle is outside the aperture at iteration " << iter << ": nothing is left to simulate" << std::endl;
					return finish(-1);
				}
			}
			if (!hip_ok(hipMemcpy(buf.data(), d_buf, cpy, hipMemcpyDeviceToHost))) return finish(-1);
			std::ofstream fout(strout + "/out" + std::to_string(iter) + '_' + std::to_string(dt) + ".bin", std::ios::out | std::ios::binary);
			if (!fout)
			{
				std::cerr << "Error: cannot write on output location. Check that \"" << strout << "\" folder exists. Create it if not." << std::endl;
				return finish(-1);
			}
			fout.write(reinterpret_cast<const char *>(buf.data()), (std::streamsize)cpy);
			if (fen)
			{
				double e3[3];
				if (!lib_ok(nbco_2d_energy_fmm(ctx, d_buf, n, d_par, e3, nullptr))) return finish(-1);
				std::fprintf(fen, "%d %.17g %.17g %.17g %.17g\n", iter, e3[0], e3[1], e3[2], e3[0] + e3[1] + e3[2]);
				std::fflush(fen);
			}
			if (fmo)
			{
				nbco_moments mom;
				if (!lib_ok(nbco_2d_beam_moments(ctx, d_buf, n, &mom))) return finish(-1);
				std::fprintf(fmo, "%d", iter);
				for (int a = 0; a < 4; ++a) std::fprintf(fmo, " %.17g", mom.mean[a]);
				for (int k = 0; k < 2; ++k)
					std::fprintf(fmo, " %.17g %.17g %.17g %.17g %.17g %.17g", std::sqrt(mom.cov[k][k]), std::sqrt(mom.cov[2 + k][2 + k]), mom.cov[k][2 + k],
					             mom.emit[k], mom.halo_q[k], mom.halo[k]);
				std::fprintf(fmo, "\n");
				std::fflush(fmo);
			}
			if (slices.on)
			{
				long long outside = 0;
				if (!lib_ok(nbco_2d_slice_moments(ctx, d_buf, n, &slices.axis, slice_recs.data(), &outside))) return finish(-1);
				if (!write_slices(strout, iter, std::to_string(dt), 2, slices.axis, slice_recs.data(), outside))
				{
					std::cerr << "Error: cannot write on output location. Check that \"" << strout << "\" folder exists. Create it if not." << std::endl;
					return finish(-1);
				}
			}
			if (sk.on)
			{
				long long n_used = 0;
				if ((!d_rho && !hip_ok(hipMalloc(&d_rho, sizeof(double) * rho_host.size()))) ||
				    !lib_ok(nbco_2d_structure_factor(ctx, d_buf, n, &sk.g, d_rho, &n_used)) ||
				    !hip_ok(hipMemcpy(rho_host.data(), d_rho, sizeof(double) * rho_host.size(), hipMemcpyDeviceToHost)))
					return finish(-1);
				if (!sklog.record(iter, std::to_string(dt), rho_host, n_used))
				{
					std::cerr << "Error: cannot write on output location. Check that \"" << strout << "\" folder exists. Create it if not." << std::endl;
					return finish(-1);
				}
			}
			if (nprobes > 0)
			{
				if (!lib_ok(nbco_2d_probe_fmm(ctx, d_buf, n, d_probes, nprobes, d_par, d_pout, d_pout + 2 * nprobes)) ||
				    !hip_ok(hipMemcpy(pout.data(), d_pout, sizeof(double) * pout.size(), hipMemcpyDeviceToHost)))
					return finish(-1);
				std::ofstream fpo(strout + "/probes" + std::to_string(iter) + '_' + std::to_string(dt) + ".bin", std::ios::out | std::ios::binary);
				if (!fpo)
				{
					std::cerr << "Error: cannot write on output location. Check that \"" << strout << "\" folder exists. Create it if not." << std::endl;
					return finish(-1);
				}
				fpo.write(reinterpret_cast<const char *>(pout.data()), (std::streamsize)(sizeof(double) * pout.size()));
			}
		}
	}
	std::cout << std::endl;
	return finish(0);
}
