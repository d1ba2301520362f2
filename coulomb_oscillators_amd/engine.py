"""ctypes binding of libnbco_hip.so (include/nbco.h).

Host-side mirror of the reference's function-pointer interface for this path:

    evaluator   void f(VEC *p, VEC *a, int n, const SCAL *param)      direct.cuh:233, fmm_cart3_kdtree.cuh:1478
    step        void step(VEC *b, const VEC *a, SCAL ds, int n)       kernel.cuh:100
    integrator  void leapfrog(f, SCAL *buf, int n, param, dt, step_func, scale)   integrator.cuh:68

Tensors are PyTorch CUDA(=HIP) tensors; only their device pointers cross the C ABI.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.environ.get("NBCO_LIB") or os.path.join(_HERE, "libnbco_hip.so")   # NBCO_LIB: A/B builds of the same ABI (diagnostics)

EVAL_DIRECT, EVAL_DIRECT_KAHAN, EVAL_FMM_KDTREE, EVAL_FMM_TRACELESS, EVAL_FMM_SYMMETRIC = 0, 1, 2, 3, 4
INTEG_EULER, INTEG_PRE_EULER, INTEG_LEAPFROG, INTEG_FORESTRUTH, INTEG_PEFRL = 0, 1, 2, 3, 4
EVAL2D_DIRECT, EVAL2D_DIRECT_KAHAN, EVAL2D_FMM = 0, 1, 2   # NBCO_2D_EVAL_* (2-D fp64 evaluators of main.cu)
REF_SEED, REF_DISCARD = 5351550349027530206, 1248     # NBCO_REF_SEED / NBCO_REF_DISCARD (main.cu:779-784)
PHASES = ["build", "p2m_m2m", "traverse", "lists", "p2p", "m2l", "l2l", "l2p", "finish", "direct", "axpy"]

KD_FIELDS = {"mult": 0, "index": 1, "splitdim": 2, "center": 3, "lbound": 4, "rbound": 5,
             "mpole": 6, "local": 7, "p2p": 8, "m2l": 9, "unsort": 10, "order": 11}


class EngineError(RuntimeError):
    """status is the NBCO_ERR_* code of include/nbco.h when the error came from the library (None otherwise)"""

    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status


ERR_UNSUPPORTED = 4   # NBCO_ERR_UNSUPPORTED


class Opts(C.Structure):
    _fields_ = [("fmm_order", C.c_int), ("tree_radius", C.c_float), ("eps2", C.c_float), ("coll", C.c_int),
                ("unsort", C.c_int), ("dens_inhom", C.c_float), ("tree_L", C.c_int), ("tree_steps", C.c_int),
                ("m2l_first", C.c_int), ("sync", C.c_int), ("list_factor", C.c_int), ("list_grow", C.c_int), ("far_fp64", C.c_int),
                ("p2p_mutual", C.c_int), ("track_order", C.c_int), ("stream", C.c_void_p)]


class KdInfo(C.Structure):
    _fields_ = [("L", C.c_int), ("ntot", C.c_int), ("order", C.c_int), ("mlt_max", C.c_int), ("n", C.c_longlong),
                ("p2p_pairs", C.c_longlong), ("m2l_pairs", C.c_longlong), ("directed_p2p", C.c_longlong),
                ("rebuilt", C.c_int), ("build_mode", C.c_int), ("p2p_halves", C.c_int), ("warm_builds", C.c_longlong), ("warm_misses", C.c_longlong),
                ("real_bytes", C.c_int), ("long_lists", C.c_int)]


class OctInfo(C.Structure):
    _fields_ = [("L", C.c_int), ("ntot", C.c_int), ("order", C.c_int), ("tpl", C.c_int), ("n", C.c_longlong),
                ("m2l_entries", C.c_longlong), ("p2p_groups", C.c_longlong), ("p2p_desc", C.c_longlong),
                ("p2p_chunks", C.c_longlong), ("real_bytes", C.c_int), ("mpole_reals", C.c_int)]


OCT_FIELDS = {"mult": 0, "index": 1, "center4": 2, "mpole": 3, "local": 4, "keys": 5, "perm": 6}


class DistLayout(C.Structure):
    _fields_ = [("world", C.c_int), ("rank", C.c_int), ("d", C.c_int), ("L", C.c_int), ("L_local", C.c_int),
                ("ntot_local", C.c_int), ("order", C.c_int), ("n_global", C.c_longlong), ("n_local", C.c_longlong),
                ("nodes_bytes", C.c_longlong), ("pos_bytes", C.c_longlong), ("csz_bytes", C.c_longlong),
                ("mpole_bytes", C.c_longlong), ("let_node_bytes", C.c_longlong), ("let_counts", C.c_int)]


class DistStep(C.Structure):
    """nbco_dist_step: the collective a distributed re-partition asks its caller to run next (include/nbco.h)"""
    _fields_ = [("op", C.c_int), ("row_bytes", C.c_int), ("send_off", C.c_longlong), ("recv_off", C.c_longlong), ("count", C.c_longlong),
                ("rows_send", C.c_longlong * 64), ("rows_recv", C.c_longlong * 64)]


class Moments(C.Structure):
    """nbco_moments: phase-space moments of a state (include/nbco.h); q = (x, y, z, vx, vy, vz), in 2-D (x, y, vx, vy)"""
    _fields_ = [("n", C.c_longlong), ("dim", C.c_int), ("mean", C.c_double * 6), ("min", C.c_double * 6), ("max", C.c_double * 6),
                ("cov", (C.c_double * 6) * 6), ("m4", (C.c_double * 5) * 3), ("emit", C.c_double * 3), ("halo_q", C.c_double * 3),
                ("halo", C.c_double * 3)]


class HistAxis(C.Structure):
    """nbco_hist_axis"""
    _fields_ = [("coord", C.c_int), ("bins", C.c_int), ("lo", C.c_double), ("hi", C.c_double)]


Q_X, Q_Y, Q_Z, Q_VX, Q_VY, Q_VZ = range(6)   # NBCO_Q_*: the coordinate of a histogram axis


class Aperture(C.Structure):
    """nbco_aperture"""
    _fields_ = [("shape", C.c_int), ("centre", C.c_double * 3), ("half", C.c_double * 3)]


AP_ELLIPSOID, AP_BOX = 0, 1   # NBCO_AP_*


class Bath(C.Structure):
    """nbco_bath: per-axis friction rates and temperatures of the Langevin bath and the 64-bit seed of its noise"""
    _fields_ = [("gamma", C.c_double * 3), ("kT", C.c_double * 3), ("seed", C.c_ulonglong)]


class BondSummary(C.Structure):
    """nbco_bond_summary (include/nbco.h)"""
    _fields_ = [("n", C.c_longlong), ("bonds", C.c_longlong), ("isolated", C.c_longlong), ("nb_max", C.c_int), ("dim", C.c_int),
                ("q_mean", C.c_double * 2), ("Q", C.c_double * 2)]


BOND_VEC = 24   # doubles of a particle's bond vector record: q^_4m in [0, 9), q^_6m in [9, 22), a_4, a_6 (include/nbco.h, nbco_bond_solid)


class SolidSummary(C.Structure):
    """nbco_solid_summary (include/nbco.h)"""
    _fields_ = [("n", C.c_longlong), ("bonds", C.c_longlong), ("isolated", C.c_longlong), ("solid_bonds", C.c_longlong), ("n_solid", C.c_longlong),
                ("xi_max", C.c_int), ("xi_min", C.c_int), ("dmin", C.c_double), ("qbar_mean", C.c_double * 2)]


class SkGrid(C.Structure):
    """nbco_sk_grid (include/nbco.h)"""
    _fields_ = [("h", C.c_int * 3), ("kstep", C.c_double * 3)]


ERR_CAPACITY = 3              # NBCO_ERR_CAPACITY

COLL_DONE, COLL_ALLREDUCE_MIN_I32, COLL_ALLREDUCE_SUM_I32, COLL_ALLGATHER, COLL_ALLTOALL = range(5)


def lib_path():
    return _LIB


def build_library(force=False):
    """Compile csrc/*.hip for gfx950 into libnbco_hip.so (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", csrc, "-s", "-j8"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return _LIB


_lib = None


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise EngineError("libnbco_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                          "there is no CPU fallback")
    L = C.CDLL(_LIB)
    P, LL, I, F, D, ULL = C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_double, C.c_ulonglong
    sig = {
        "nbco_opts_default": [C.POINTER(Opts)],
        "nbco_create": [C.POINTER(P), C.POINTER(Opts)],
        "nbco_destroy": [P],
        "nbco_set_opts": [P, C.POINTER(Opts)],
        "nbco_get_opts": [P, C.POINTER(Opts)],
        "nbco_sync": [P],
        "nbco_step": [P, P, P, F, LL],
        "nbco_add_elastic": [P, P, P, LL, P],
        "nbco_elastic": [P, P, P, LL, P],
        "nbco_rescale": [P, P, LL, P],
        "nbco_gather": [P, P, P, P, LL],
        "nbco_gather_inverse": [P, P, P, P, LL],
        "nbco_copy": [P, P, P, LL],
        "nbco_direct": [P, P, P, LL, P],
        "nbco_direct3": [P, P, P, LL, P],
        "nbco_fmm_kdtree": [P, P, P, LL, P],
        "nbco_fmm_traceless": [P, P, P, LL, P],
        "nbco_fmm_symmetric": [P, P, P, LL, P],
        "nbco_fmm_oct_shard": [P, P, P, LL, P, I, I, I, C.POINTER(LL)],
        "nbco_force": [P, I, P, LL, P, I],
        "nbco_integrate": [P, I, I, P, LL, P, D, D, I],
        "nbco_integrate_steps": [P, I, I, P, LL, P, D, D, I, I],
        "nbco_helix_matrices": [C.POINTER(D), D, C.POINTER(D), C.POINTER(D)],
        "nbco_2d_helix_matrices": [D, D, C.POINTER(D), C.POINTER(D)],
        "nbco_drift_b": [P, P, P, LL, C.POINTER(D), D],
        "nbco_integrate_b": [P, I, I, P, LL, P, D, D, I, C.POINTER(D)],
        "nbco_integrate_steps_b": [P, I, I, P, LL, P, D, D, I, I, C.POINTER(D)],
        "nbco_2d_drift_b": [P, P, P, LL, D, D],
        "nbco_2d_integrate_b": [P, I, I, P, LL, P, D, D, I, D],
        "nbco_2d_integrate_steps_b": [P, I, I, P, LL, P, D, D, I, I, D],
        "nbco_bath_coeffs": [C.POINTER(Bath), D, C.POINTER(D), C.POINTER(D)],
        "nbco_bath_apply": [P, P, LL, C.POINTER(Bath), D, I, ULL],
        "nbco_integrate_t": [P, I, I, P, LL, P, D, D, I, C.POINTER(D), C.POINTER(Bath), ULL],
        "nbco_integrate_steps_t": [P, I, I, P, LL, P, D, D, I, I, C.POINTER(D), C.POINTER(Bath), ULL],
        "nbco_2d_bath_apply": [P, P, LL, C.POINTER(Bath), D, I, ULL],
        "nbco_2d_integrate_t": [P, I, I, P, LL, P, D, D, I, D, C.POINTER(Bath), ULL],
        "nbco_2d_integrate_steps_t": [P, I, I, P, LL, P, D, D, I, I, D, C.POINTER(Bath), ULL],
        "nbco_minmax": [P, P, LL, P],
        "nbco_mean_relerr": [P, P, P, LL, C.POINTER(F)],
        "nbco_pow_sum": [P, P, I, LL, C.POINTER(D)],
        "nbco_energy": [P, P, LL, P, C.POINTER(D)],
        "nbco_energy_fmm": [P, P, LL, P, C.POINTER(D)],
        "nbco_kd_potential": [P, P, LL, P, C.POINTER(D), P],
        "nbco_energy_tree": [P, P, LL, P, C.POINTER(D), P],
        "nbco_probe": [P, P, LL, P, LL, P, P, P],
        "nbco_probe_tree": [P, P, LL, P, LL, P, P, P],
        "nbco_kd_probe": [P, P, LL, P, P, P],
        "nbco_kd_get_info": [P, C.POINTER(KdInfo)],
        "nbco_kd_copy": [P, I, P, LL],
        "nbco_oct_get_info": [P, C.POINTER(OctInfo)],
        "nbco_oct_copy": [P, I, P, LL],
        "nbco_dist_layout_query": [P, LL, I, I, C.POINTER(DistLayout)],
        "nbco_dist_partition": [P, P, LL, I, I, P],
        "nbco_dist_local": [P, P, LL, P, P],
        "nbco_dist_local_build": [P, P, LL, P],
        "nbco_dist_local_upward": [P, P, LL, P],
        "nbco_dist_finish": [P, P, P, P, P, P],
        "nbco_dist_local_geom": [P, P, LL, P, P],
        "nbco_dist_local_mpole": [P, P, LL, P],
        "nbco_dist_finish_traverse": [P, P, P],
        "nbco_dist_finish_rest": [P, P, P, P, P],
        "nbco_dist_repartition_workspace": [P, LL, I, C.POINTER(LL)],
        "nbco_dist_repartition_begin": [P, P, LL, I, I, P, LL, C.POINTER(DistStep)],
        "nbco_dist_repartition_next": [P, C.POINTER(DistStep)],
        "nbco_dist_let_local_geom": [P, P, LL, P],
        "nbco_dist_let_local_mpole": [P, P, LL],
        "nbco_dist_let_select": [P, P, P],
        "nbco_dist_let_pack": [P, P, P, P],
        "nbco_dist_let_finish": [P, P, P, P, P, P, P],
        "nbco_dist_let_check": [P],
        "nbco_dist_let_pack_capped": [P, P, P, P],
        "nbco_dist_let_finish_capped": [P, P, P, P, P, P, P],
        "nbco_dist_let_settle": [P, I],
        "nbco_dist_turnaround": [P, P, LL, P, D, D, I],
        "nbco_aux_stream": [P, C.POINTER(C.c_void_p)],
        "nbco_debug_violations": [P, C.POINTER(LL)],
        "nbco_profile_enable": [P, I],
        "nbco_profile_reset": [P],
        "nbco_profile_get": [P, I, C.POINTER(D), C.POINTER(LL)],
        "nbco_2d_direct": [P, P, P, LL, P],
        "nbco_2d_direct3": [P, P, P, LL, P],
        "nbco_2d_fmm": [P, P, P, LL, P],
        "nbco_2d_force": [P, I, P, LL, P, I],
        "nbco_2d_integrate": [P, I, I, P, LL, P, D, D, I],
        "nbco_2d_integrate_steps": [P, I, I, P, LL, P, D, D, I, I],
        "nbco_2d_mean_relerr": [P, P, P, LL, C.POINTER(D)],
        "nbco_2d_energy": [P, P, LL, P, C.POINTER(D), P],
        "nbco_2d_energy_fmm": [P, P, LL, P, C.POINTER(D), P],
        "nbco_2d_probe": [P, P, LL, P, LL, P, P, P],
        "nbco_2d_probe_fmm": [P, P, LL, P, LL, P, P, P],
        "nbco_beam_moments": [P, P, LL, C.POINTER(Moments)],
        "nbco_2d_beam_moments": [P, P, LL, C.POINTER(Moments)],
        "nbco_moments_derive": [C.POINTER(Moments)],
        "nbco_hist": [P, P, LL, C.POINTER(HistAxis), I, P],
        "nbco_2d_hist": [P, P, LL, C.POINTER(HistAxis), I, P],
        "nbco_slice_moments": [P, P, LL, C.POINTER(HistAxis), C.POINTER(Moments), C.POINTER(LL)],
        "nbco_2d_slice_moments": [P, P, LL, C.POINTER(HistAxis), C.POINTER(Moments), C.POINTER(LL)],
        "nbco_pair_hist": [P, P, LL, I, D, P, P],
        "nbco_pair_hist_tree": [P, P, LL, I, D, P, P],
        "nbco_2d_pair_hist": [P, P, LL, I, D, P, P],
        "nbco_bond_harmonics": [C.POINTER(D), C.POINTER(D), C.POINTER(D)],
        "nbco_bond_order": [P, P, LL, D, P, P, C.POINTER(BondSummary)],
        "nbco_bond_order_tree": [P, P, LL, D, P, P, C.POINTER(BondSummary)],
        "nbco_2d_bond_order": [P, P, LL, D, P, P, C.POINTER(BondSummary)],
        "nbco_bond_coherence": [C.POINTER(D), C.POINTER(D), C.POINTER(D)],
        "nbco_bond_vectors": [P, P, LL, D, P, P],
        "nbco_bond_vectors_tree": [P, P, LL, D, P, P],
        "nbco_bond_solid": [P, P, LL, D, P, D, C.c_int, P, P, P, C.POINTER(SolidSummary)],
        "nbco_bond_solid_tree": [P, P, LL, D, P, D, C.c_int, P, P, P, C.POINTER(SolidSummary)],
        "nbco_structure_factor": [P, P, LL, C.POINTER(SkGrid), P, C.POINTER(LL)],
        "nbco_2d_structure_factor": [P, P, LL, C.POINTER(SkGrid), P, C.POINTER(LL)],
        "nbco_sk_phase": [D, C.POINTER(D)],
        "nbco_traj_record": [P, P, LL, P, P, LL, I, I, I],
        "nbco_time_corr": [P, P, LL, I, I, I, P],
        "nbco_time_corr_derive": [P, I, P],
        "nbco_modes_record": [P, P, LL, C.POINTER(SkGrid), P, I, I, C.POINTER(LL)],
        "nbco_mode_corr": [P, P, C.POINTER(SkGrid), I, I, I, P],
        "nbco_mode_corr_ref": [P, C.POINTER(SkGrid), I, I, I, P],
        "nbco_mode_corr_derive": [P, C.POINTER(SkGrid), I, D, P],
        "nbco_aperture_count": [P, P, LL, C.POINTER(Aperture), C.POINTER(LL)],
        "nbco_aperture_apply": [P, P, LL, C.POINTER(Aperture), C.POINTER(LL), P, P, LL],
        "nbco_2d_aperture_count": [P, P, LL, C.POINTER(Aperture), C.POINTER(LL)],
        "nbco_2d_aperture_apply": [P, P, LL, C.POINTER(Aperture), C.POINTER(LL), P, P, LL],
        "nbco_2d_init_kv": [P, LL, P, P, C.c_ulonglong, C.c_ulonglong],
        "nbco_2d_init_gaussian": [P, LL, P, P, C.c_ulonglong, C.c_ulonglong],
    }
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = I
    L.nbco_last_error.argtypes = [P]
    L.nbco_last_error.restype = C.c_char_p
    _lib = L
    return L


_genops = None


def genops_lib():
    """libnbco_genops_host.so: the generated far-field operator bodies compiled for the host (csrc/genops_host.cpp).  Signatures are
    set for the potential operator nbco_genop_lpot_f32 / _f64(order, Lp, d, out); needs no GPU."""
    global _genops
    if _genops is None:
        path = os.path.join(_HERE, "libnbco_genops_host.so")
        if not os.path.exists(path):
            raise EngineError("libnbco_genops_host.so is not built (make -C coulomb_oscillators_amd/csrc)")
        G = C.CDLL(path)
        for name in ("nbco_genop_lpot_f32", "nbco_genop_lpot_f64"):
            fn = getattr(G, name)
            fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
            fn.restype = C.c_int
        _genops = G
    return _genops


def init2d(n, kind="kv", a=None, b=None, seed=REF_SEED, discard=REF_DISCARD):
    """Host initial state of main.cu (nbco_2d_init_kv / nbco_2d_init_gaussian): numpy float64 [2, n, 2] = [positions, velocities].
    kind "kv": a = semi-axes A, b = depressed phase advances omega; "ga": a = position std x, b = velocity std u.  Needs no GPU."""
    import numpy as np
    out = np.zeros((2, n, 2), dtype=np.float64)
    a2 = (C.c_double * 2)(*a)
    b2 = (C.c_double * 2)(*b)
    fn = _load().nbco_2d_init_kv if kind == "kv" else _load().nbco_2d_init_gaussian
    rc = fn(out.ctypes.data_as(C.c_void_p), n, C.cast(a2, C.c_void_p), C.cast(b2, C.c_void_p), seed, discard)
    if rc != 0:
        raise EngineError("nbco_2d_init_%s failed with status %d" % (kind, rc), status=rc)
    return out


def _omega3(omega):
    return None if omega is None else (C.c_double * 3)(*[float(w) for w in omega])


def helix_matrices(omega, s):
    """(R, A), float64 3 x 3: the helix drift of a uniform magnetic field Omega = omega over s, v <- R v, x <- x + A v with the old v
    (nbco_helix_matrices, include/nbco.h).  Host only, needs no GPU; the one place the matrices are formed."""
    import numpy as np
    R, A = (C.c_double * 9)(), (C.c_double * 9)()
    rc = _load().nbco_helix_matrices(_omega3(omega), float(s), R, A)
    if rc != 0:
        raise EngineError("nbco_helix_matrices failed with status %d" % rc, status=rc)
    return np.array(R[:], dtype=np.float64).reshape(3, 3), np.array(A[:], dtype=np.float64).reshape(3, 3)


def helix_matrices_2d(omega, s):
    """the 2-D form: omega a scalar (the field points out of the plane), (R, A) float64 2 x 2 (nbco_2d_helix_matrices)"""
    import numpy as np
    R, A = (C.c_double * 4)(), (C.c_double * 4)()
    rc = _load().nbco_2d_helix_matrices(float(omega), float(s), R, A)
    if rc != 0:
        raise EngineError("nbco_2d_helix_matrices failed with status %d" % rc, status=rc)
    return np.array(R[:], dtype=np.float64).reshape(2, 2), np.array(A[:], dtype=np.float64).reshape(2, 2)


def _bath(gamma, kT, seed):
    """nbco_bath from per-axis rates and temperatures (two or three values each; a scalar serves every axis) and a 64-bit seed"""
    def three(q):
        q = [float(q)] * 3 if not hasattr(q, "__len__") else [float(t) for t in q]
        return q + [0.0] * (3 - len(q))
    return Bath((C.c_double * 3)(*three(gamma)), (C.c_double * 3)(*three(kT)), int(seed) & 0xFFFFFFFFFFFFFFFF)


def bath_coeffs(gamma, kT, s):
    """(c1, c2), float64[3]: the coefficients of the exact Langevin bath step over s, v' = c1 v + c2 xi with c1 = exp(-gamma s) and
    c2 = sqrt(kT (1 - exp(-2 gamma s))) (nbco_bath_coeffs, include/nbco.h).  Host only, needs no GPU; the one place they are formed."""
    import numpy as np
    c1, c2 = (C.c_double * 3)(), (C.c_double * 3)()
    rc = _load().nbco_bath_coeffs(C.byref(_bath(gamma, kT, 0)), float(s), c1, c2)
    if rc != 0:
        raise EngineError("nbco_bath_coeffs failed with status %d" % rc, status=rc)
    return np.array(c1[:], dtype=np.float64), np.array(c2[:], dtype=np.float64)


def bond_harmonics(u):
    """(y4, y6), float64[9] and float64[13]: the orthonormal real spherical harmonics of degree 4 and 6 at the unit vector u, as the
    bond-order kernels form them (nbco_bond_harmonics, include/nbco.h): entry 0 is m = 0, 2m - 1 and 2m the cosine and sine parts
    of m.  u is taken as it is.  Host only, needs no GPU; the one place they are formed."""
    import numpy as np
    u3 = (C.c_double * 3)(*[float(t) for t in u])
    y4, y6 = (C.c_double * 9)(), (C.c_double * 13)()
    rc = _load().nbco_bond_harmonics(u3, y4, y6)
    if rc != 0:
        raise EngineError("nbco_bond_harmonics failed with status %d" % rc, status=rc)
    return np.array(y4[:], dtype=np.float64), np.array(y6[:], dtype=np.float64)


def bond_coherence(vec_i, vec_j):
    """d6 of a bond from the bond vector records (BOND_VEC doubles each) of its two ends, as the solid-bond kernels form it
    (nbco_bond_coherence, include/nbco.h): the products of the 13 q^_6 entries added from the left, every product and sum rounded once.
    Host only, needs no GPU."""
    a, b = (C.c_double * BOND_VEC)(*[float(t) for t in vec_i]), (C.c_double * BOND_VEC)(*[float(t) for t in vec_j])
    d6 = C.c_double()
    rc = _load().nbco_bond_coherence(a, b, C.byref(d6))
    if rc != 0:
        raise EngineError("nbco_bond_coherence failed with status %d" % rc, status=rc)
    return d6.value


def sk_phase(t):
    """(cos 2 pi t, sin 2 pi t) as the structure-factor kernels form the phase of t cycles (nbco_sk_phase, include/nbco.h): an exact
    reduction and fixed polynomials, no libm.  Host only, needs no GPU; the one place it is formed."""
    cs = (C.c_double * 2)()
    rc = _load().nbco_sk_phase(float(t), cs)
    if rc != 0:
        raise EngineError("nbco_sk_phase failed with status %d" % rc, status=rc)
    return cs[0], cs[1]


CORR_LAG = [("dx2", "<f8", (3,)), ("r4", "<f8"), ("vv", "<f8", (3,)), ("pairs", "<u8")]   # nbco_corr_lag as a numpy record, 64 bytes


def time_corr_derive(rec):
    """msd_x msd_y msd_z msd alpha2 vacf_x vacf_y vacf_z per lag from the raw sums of Engine.time_corr (nbco_time_corr_derive,
    include/nbco.h): rec a device tensor as time_corr returns it, or a numpy array of CORR_LAG records or of lags x 8 float64 holding
    them.  Returns a float64 array lags x 8.  A lag without pairs gives zeros, msd == 0 gives alpha2 = 0.  Host only, needs no GPU."""
    import numpy as np
    if hasattr(rec, "cpu"):
        rec = rec.cpu().numpy()
    raw = np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 64)
    out = np.empty((raw.shape[0], 8), dtype=np.float64)
    rc = _load().nbco_time_corr_derive(raw.ctypes.data_as(C.c_void_p), raw.shape[0], out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise EngineError("nbco_time_corr_derive failed with status %d" % rc, status=rc)
    return out


MODE_LAG = [("rr", "<f8"), ("ll", "<f8"), ("jj", "<f8"), ("s0", "<f8", (2,)), ("s1", "<f8", (2,)), ("pairs", "<u8")]   # nbco_mode_lag as a numpy record, 64 bytes


def _sk_grid(h, kstep, dim=3):
    g = SkGrid()
    for a in range(dim):
        g.h[a] = int(h[a])
        g.kstep[a] = float(kstep[a])
    return g


def _sk_count(h):
    """K of a 3-D grid, 0 for an h the library refuses (nothing is sized by a bad h)"""
    if not all(0 <= int(h[a]) <= 64 for a in range(3)):
        return 0
    return (int(h[0]) + 1) * (2 * int(h[1]) + 1) * (2 * int(h[2]) + 1)


def mode_corr_ref(series, h, kstep, frames, lags):
    """the raw sums of Engine.mode_corr formed on the host by the same rule (nbco_mode_corr_ref, include/nbco.h): series a float64
    numpy array K x frames_cap x 8 of mode records.  Returns a numpy array K x lags of MODE_LAG records with the bytes the device
    returns for the same series.  Host only, needs no GPU."""
    import numpy as np
    series = np.ascontiguousarray(series, dtype=np.float64)
    K = _sk_count(h)
    if series.ndim != 3 or series.shape[0] != K or series.shape[2] != 8:
        raise EngineError("mode_corr_ref: series must be K x frames_cap x 8 for this grid", status=1)
    out = np.zeros((K, max(int(lags), 0)), dtype=MODE_LAG)
    g = _sk_grid(h, kstep)
    rc = _load().nbco_mode_corr_ref(series.ctypes.data_as(C.c_void_p), C.byref(g), int(series.shape[1]), int(frames), int(lags), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise EngineError("nbco_mode_corr_ref failed with status %d" % rc, status=rc)
    return out


def mode_corr_derive(rec, h, kstep, n_norm):
    """F, F_c, C_L, C_T per (k, lag) from the raw sums of Engine.mode_corr (nbco_mode_corr_derive, include/nbco.h): rec a device tensor
    as mode_corr returns it, or a numpy array K x lags of MODE_LAG records (or K x lags x 8 float64 holding them).  Returns a float64
    array K x lags x 4.  pairs == 0 or n_norm <= 0 gives zeros, k = 0 gives C_L = C_T = 0.  Host only, needs no GPU."""
    import numpy as np
    if hasattr(rec, "cpu"):
        rec = rec.cpu().numpy()
    K = _sk_count(h)
    raw = np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 64)
    if K == 0 or raw.shape[0] % K != 0:
        raise EngineError("mode_corr_derive: rec must hold K x lags records for this grid", status=1)
    lags = raw.shape[0] // K
    out = np.empty((K, lags, 4), dtype=np.float64)
    g = _sk_grid(h, kstep)
    rc = _load().nbco_mode_corr_derive(raw.ctypes.data_as(C.c_void_p), C.byref(g), lags, float(n_norm), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise EngineError("nbco_mode_corr_derive failed with status %d" % rc, status=rc)
    return out


def default_opts(**kw):
    o = Opts()
    _load().nbco_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Engine:
    """One nbco context bound to the current torch HIP device and stream."""

    def __init__(self, stream=None, **opts):
        import torch
        self.lib = _load()
        if not torch.cuda.is_available():
            raise EngineError("no HIP device visible to PyTorch; the engine has no CPU fallback")
        self.torch = torch
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        o = default_opts(**opts)
        o.stream = stream
        self.ctx = C.c_void_p()
        rc = self.lib.nbco_create(C.byref(self.ctx), C.byref(o))
        if rc != 0:
            raise EngineError("nbco_create failed with status %d" % rc)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.nbco_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise EngineError("nbco status %d: %s" % (rc, self.lib.nbco_last_error(self.ctx).decode()), status=rc)

    # ---- options --------------------------------------------------------------------------------
    def opts(self):
        o = Opts()
        self._chk(self.lib.nbco_get_opts(self.ctx, C.byref(o)))
        return o

    def set(self, **kw):
        o = self.opts()
        for k, v in kw.items():
            setattr(o, k, v)
        self._chk(self.lib.nbco_set_opts(self.ctx, C.byref(o)))

    def sync(self):
        self._chk(self.lib.nbco_sync(self.ctx))

    # ---- basic kernels --------------------------------------------------------------------------
    def step(self, b, a, ds, n=None):
        n = b.numel() // 3 if n is None else n
        self._chk(self.lib.nbco_step(self.ctx, _ptr(b), _ptr(a), ds, n))

    def add_elastic(self, p, a, n, k=None):
        self._chk(self.lib.nbco_add_elastic(self.ctx, _ptr(p), _ptr(a), n, _ptr(k)))

    def elastic(self, p, a, n, k=None):
        self._chk(self.lib.nbco_elastic(self.ctx, _ptr(p), _ptr(a), n, _ptr(k)))

    def rescale(self, a, n, param):
        self._chk(self.lib.nbco_rescale(self.ctx, _ptr(a), n, _ptr(param)))

    def gather(self, dst, src, idx, n):
        self._chk(self.lib.nbco_gather(self.ctx, _ptr(dst), _ptr(src), _ptr(idx), n))

    def gather_inverse(self, dst, src, idx, n):
        self._chk(self.lib.nbco_gather_inverse(self.ctx, _ptr(dst), _ptr(src), _ptr(idx), n))

    def copy(self, dst, src, n):
        self._chk(self.lib.nbco_copy(self.ctx, _ptr(dst), _ptr(src), n))

    # ---- evaluators: f(p, a, n, param) -----------------------------------------------------------
    def direct(self, p, a, n, param=None):
        self._chk(self.lib.nbco_direct(self.ctx, _ptr(p), _ptr(a), n, _ptr(param)))

    def direct3(self, p, a, n, param=None):
        self._chk(self.lib.nbco_direct3(self.ctx, _ptr(p), _ptr(a), n, _ptr(param)))

    def fmm_cart3_kdtree(self, p, a, n, param=None):
        self._chk(self.lib.nbco_fmm_kdtree(self.ctx, _ptr(p), _ptr(a), n, _ptr(param)))

    def fmm_cart3_traceless(self, p, a, n, param=None):
        self._chk(self.lib.nbco_fmm_traceless(self.ctx, _ptr(p), _ptr(a), n, _ptr(param)))

    def fmm_cart3(self, p, a, n, param=None):
        """the uniform-octree evaluator with symmetric multipoles (fmm_cart3_symmetric.cuh:413)"""
        self._chk(self.lib.nbco_fmm_symmetric(self.ctx, _ptr(p), _ptr(a), n, _ptr(param)))

    def fmm_oct_shard(self, p, a, n, param, world, rank, symmetric=False):
        """this rank's slab of the uniform-octree evaluation (nbco_fmm_oct_shard); returns the particle boundaries of all slabs"""
        b = (C.c_longlong * (world + 1))()
        self._chk(self.lib.nbco_fmm_oct_shard(self.ctx, _ptr(p), _ptr(a), n, _ptr(param), int(symmetric), world, rank, b))
        return list(b)

    def compute_force(self, kind, buf, n, param, elastic=True):
        self._chk(self.lib.nbco_force(self.ctx, kind, _ptr(buf), n, _ptr(param), int(elastic)))

    def integrate(self, scheme, kind, buf, n, param, dt, scale=1.0, elastic=True):
        self._chk(self.lib.nbco_integrate(self.ctx, scheme, kind, _ptr(buf), n, _ptr(param), dt, scale, int(elastic)))

    def integrate_steps(self, scheme, kind, buf, n, param, dt, steps, scale=1.0, elastic=True):
        """`steps` steps in one call (nbco_integrate_steps): same final state as `steps` calls of integrate()"""
        self._chk(self.lib.nbco_integrate_steps(self.ctx, scheme, kind, _ptr(buf), n, _ptr(param), dt, scale, int(elastic), int(steps)))

    # ---- uniform magnetic field: the drift along a helix (include/nbco.h) ---------------------------------------------------
    helix_matrices = staticmethod(helix_matrices)
    helix_matrices_2d = staticmethod(helix_matrices_2d)

    def drift_b(self, x, v, n, omega, s):
        """the helix drift of n particles in the uniform field omega = (wx, wy, wz) over s (nbco_drift_b): x and v are float32 device
        tensors of xyz triplets, both rewritten from the old v"""
        self._chk(self.lib.nbco_drift_b(self.ctx, _ptr(x), _ptr(v), n, _omega3(omega), float(s)))

    def integrate_b(self, scheme, kind, buf, n, param, dt, omega, scale=1.0, elastic=True):
        """integrate() with the drift replaced by the helix drift of the uniform field omega, in radians per unit of dt
        (nbco_integrate_b); omega = (0, 0, 0) is integrate() itself"""
        self._chk(self.lib.nbco_integrate_b(self.ctx, scheme, kind, _ptr(buf), n, _ptr(param), dt, scale, int(elastic), _omega3(omega)))

    def integrate_steps_b(self, scheme, kind, buf, n, param, dt, steps, omega, scale=1.0, elastic=True):
        """`steps` steps in one call (nbco_integrate_steps_b): same final state as `steps` calls of integrate_b()"""
        self._chk(self.lib.nbco_integrate_steps_b(self.ctx, scheme, kind, _ptr(buf), n, _ptr(param), dt, scale, int(elastic), int(steps), _omega3(omega)))

    def drift_b_2d(self, x, v, n, omega, s):
        """the 2-D form: float64 xy pairs, omega a scalar (nbco_2d_drift_b)"""
        self._chk(self.lib.nbco_2d_drift_b(self.ctx, _ptr(x), _ptr(v), n, float(omega), float(s)))

    def integrate_b_2d(self, scheme, kind, buf, n, param, dt, omega, scale=1.0, elastic=True):
        self._chk(self.lib.nbco_2d_integrate_b(self.ctx, scheme, kind, _ptr(buf), n, _ptr(param), dt, scale, int(elastic), float(omega)))

    def integrate_steps_b_2d(self, scheme, kind, buf, n, param, dt, steps, omega, scale=1.0, elastic=True):
        self._chk(self.lib.nbco_2d_integrate_steps_b(self.ctx, scheme, kind, _ptr(buf), n, _ptr(param), dt, scale, int(elastic), int(steps), float(omega)))

    # ---- Langevin bath: the exact friction-and-noise step of the velocities (include/nbco.h) ------------------------------------
    bath_coeffs = staticmethod(bath_coeffs)

    def bath_apply(self, v, n, gamma, kT, s, half, tick, seed=REF_SEED):
        """O(s) alone on the float32 velocities v of n particles (nbco_bath_apply): v' = c1 v + c2 xi per row and axis, the noise keyed by
        (seed, tick, half, row, axis); gamma and kT per axis"""
        self._chk(self.lib.nbco_bath_apply(self.ctx, _ptr(v), n, C.byref(_bath(gamma, kT, seed)), float(s), int(half), int(tick)))

    def integrate_t(self, scheme, kind, buf, n, param, dt, gamma, kT, tick, seed=REF_SEED, omega=None, scale=1.0, elastic=True):
        """integrate() or integrate_b() (omega given) wrapped in the two half bath steps O(dt/2) (nbco_integrate_t); every gamma 0 is the
        counterpart itself"""
        self._chk(self.lib.nbco_integrate_t(self.ctx, scheme, kind, _ptr(buf), n, _ptr(param), dt, scale, int(elastic), _omega3(omega),
                                            C.byref(_bath(gamma, kT, seed)), int(tick)))

    def integrate_steps_t(self, scheme, kind, buf, n, param, dt, steps, gamma, kT, tick0, seed=REF_SEED, omega=None, scale=1.0, elastic=True):
        """`steps` steps in one call, step k at tick0 + k (nbco_integrate_steps_t): same final state as `steps` calls of integrate_t()"""
        self._chk(self.lib.nbco_integrate_steps_t(self.ctx, scheme, kind, _ptr(buf), n, _ptr(param), dt, scale, int(elastic), int(steps), _omega3(omega),
                                                  C.byref(_bath(gamma, kT, seed)), int(tick0)))

    def bath_apply_2d(self, v, n, gamma, kT, s, half, tick, seed=REF_SEED):
        """the 2-D form: float64 xy pairs, gamma and kT two values each (nbco_2d_bath_apply)"""
        self._chk(self.lib.nbco_2d_bath_apply(self.ctx, _ptr(v), n, C.byref(_bath(gamma, kT, seed)), float(s), int(half), int(tick)))

    def integrate_t_2d(self, scheme, kind, buf, n, param, dt, gamma, kT, tick, seed=REF_SEED, omega=0.0, scale=1.0, elastic=True):
        self._chk(self.lib.nbco_2d_integrate_t(self.ctx, scheme, kind, _ptr(buf), n, _ptr(param), dt, scale, int(elastic), float(omega),
                                               C.byref(_bath(gamma, kT, seed)), int(tick)))

    def integrate_steps_t_2d(self, scheme, kind, buf, n, param, dt, steps, gamma, kT, tick0, seed=REF_SEED, omega=0.0, scale=1.0, elastic=True):
        self._chk(self.lib.nbco_2d_integrate_steps_t(self.ctx, scheme, kind, _ptr(buf), n, _ptr(param), dt, scale, int(elastic), int(steps), float(omega),
                                                     C.byref(_bath(gamma, kT, seed)), int(tick0)))

    # ---- 2-D fp64 evaluators (main.cu): float64 tensors, xy pairs, param = {xi/N, 0, kx, ky} -------------------------------
    def direct_2d(self, p, a, n, param=None):
        self._chk(self.lib.nbco_2d_direct(self.ctx, _ptr(p), _ptr(a), n, _ptr(param)))

    def direct3_2d(self, p, a, n, param=None):
        self._chk(self.lib.nbco_2d_direct3(self.ctx, _ptr(p), _ptr(a), n, _ptr(param)))

    def fmm_2d(self, p, a, n, param):
        """fmm_cart: p holds positions then velocities (2n xy pairs); both are left in cell order"""
        self._chk(self.lib.nbco_2d_fmm(self.ctx, _ptr(p), _ptr(a), n, _ptr(param)))

    def compute_force_2d(self, kind, buf, n, param, elastic=True):
        self._chk(self.lib.nbco_2d_force(self.ctx, kind, _ptr(buf), n, _ptr(param), int(elastic)))

    def integrate_2d(self, scheme, kind, buf, n, param, dt, scale=1.0, elastic=True):
        self._chk(self.lib.nbco_2d_integrate(self.ctx, scheme, kind, _ptr(buf), n, _ptr(param), dt, scale, int(elastic)))

    def integrate_steps_2d(self, scheme, kind, buf, n, param, dt, steps, scale=1.0, elastic=True):
        self._chk(self.lib.nbco_2d_integrate_steps(self.ctx, scheme, kind, _ptr(buf), n, _ptr(param), dt, scale, int(elastic), int(steps)))

    def mean_relerr_2d(self, x, ref, n):
        out = C.c_double()
        self._chk(self.lib.nbco_2d_mean_relerr(self.ctx, _ptr(x), _ptr(ref), n, C.byref(out)))
        return out.value

    def _energy_2d(self, fn, buf, n, param, phi):
        import numpy as np
        out = (C.c_double * 3)()
        self._chk(fn(self.ctx, _ptr(buf), n, _ptr(param), out, _ptr(phi)))
        return np.array(out[:], dtype=np.float64)

    def energy_2d(self, buf, n, param, phi=None):
        """{kinetic, elastic, coulomb} of buf = [pos n | vel n | ..] with the exact O(N^2) pair potential (nbco_2d_energy); phi: None
        or a float64 device tensor of n elements that receives psi_i in buf's particle order.  buf is not modified."""
        return self._energy_2d(self.lib.nbco_2d_energy, buf, n, param, phi)

    def energy_fmm_2d(self, buf, n, param, phi=None):
        """the same with the Coulomb part from an O(N) quadtree FMM potential pass of its own (nbco_2d_energy_fmm): no preceding
        evaluation is needed, buf is neither modified nor reordered"""
        return self._energy_2d(self.lib.nbco_2d_energy_fmm, buf, n, param, phi)

    def probe_2d(self, p, n, t, m, param, a=None, psi=None):
        """field and potential of the n sources p at the m probes t, exact O(n m) sums (nbco_2d_probe): a receives m xy pairs, psi m
        values, float64 device tensors in the probes' order; either may be None, not both.  Every source counts (no self exclusion),
        t may be p, and neither is modified."""
        self._chk(self.lib.nbco_2d_probe(self.ctx, _ptr(p), n, _ptr(t), m, _ptr(param), _ptr(a), _ptr(psi)))

    def probe_fmm_2d(self, p, n, t, m, param, a=None, psi=None):
        """the same from the quadtree nbco_2d_fmm would build for p, the multipoles evaluated at the probes (nbco_2d_probe_fmm)"""
        self._chk(self.lib.nbco_2d_probe_fmm(self.ctx, _ptr(p), n, _ptr(t), m, _ptr(param), _ptr(a), _ptr(psi)))

    # ---- reductions -----------------------------------------------------------------------------
    def minmax(self, p, n):
        out = self.torch.empty(6, dtype=self.torch.float32, device=p.device)
        self._chk(self.lib.nbco_minmax(self.ctx, _ptr(p), n, _ptr(out)))
        return out.view(2, 3)

    def mean_relerr(self, x, ref, n):
        out = C.c_float()
        self._chk(self.lib.nbco_mean_relerr(self.ctx, _ptr(x), _ptr(ref), n, C.byref(out)))
        return out.value

    def pow_sum(self, x, expo, n):
        out = (C.c_double * 3)()
        self._chk(self.lib.nbco_pow_sum(self.ctx, _ptr(x), expo, n, out))
        return list(out)

    def energy(self, buf, n, param):
        out = (C.c_double * 3)()
        self._chk(self.lib.nbco_energy(self.ctx, _ptr(buf), n, _ptr(param), out))
        return list(out)

    def energy_fmm(self, buf, n, param):
        """{kinetic, elastic, coulomb} with the Coulomb part from the lists of the last kd-tree evaluation (O(N log N))"""
        out = (C.c_double * 3)()
        self._chk(self.lib.nbco_energy_fmm(self.ctx, _ptr(buf), n, _ptr(param), out))
        return list(out)

    def energy_kd(self, buf, n, param, phi=None):
        """{kinetic, elastic, coulomb} with the Coulomb part from the locals of the last kd-tree evaluation, O(N) (nbco_kd_potential; the
        preconditions of energy_fmm); phi: None or a float64 device tensor of n elements that receives psi_i in buf's particle order"""
        return self._energy_2d(self.lib.nbco_kd_potential, buf, n, param, phi)

    def energy_tree(self, buf, n, param, phi=None):
        """the same from a kd-tree evaluation of its own on a private context (nbco_energy_tree): valid in any state of this engine,
        which it leaves untouched; buf is neither modified nor reordered"""
        return self._energy_2d(self.lib.nbco_energy_tree, buf, n, param, phi)

    def probe(self, p, n, t, m, param, a=None, psi=None):
        """field and potential of the n sources p at the m probes t, exact O(n m) sums (nbco_probe): p and t are float32 device tensors
        of xyz triplets, a receives m xyz triplets, psi m values, float64 device tensors in the probes' order; either may be None, not
        both.  Every source counts (no self exclusion), t may be p, and neither is modified."""
        self._chk(self.lib.nbco_probe(self.ctx, _ptr(p), n, _ptr(t), m, _ptr(param), _ptr(a), _ptr(psi)))

    def probe_kd(self, t, m, param, a=None, psi=None):
        """the same from a walk over the tree and multipoles of the last kd-tree evaluation (nbco_kd_probe; the preconditions of
        energy_fmm): accepted inner nodes by their expansions at the probe, leaves always pair by pair"""
        self._chk(self.lib.nbco_kd_probe(self.ctx, _ptr(t), m, _ptr(param), _ptr(a), _ptr(psi)))

    def probe_tree(self, p, n, t, m, param, a=None, psi=None):
        """the same from a kd-tree of its own on a private context (nbco_probe_tree): valid in any state of this engine, which it
        leaves untouched; p is neither modified nor reordered"""
        self._chk(self.lib.nbco_probe_tree(self.ctx, _ptr(p), n, _ptr(t), m, _ptr(param), _ptr(a), _ptr(psi)))

    # ---- beam diagnostics ------------------------------------------------------------------------
    def _moments(self, fn, buf, n):
        out = Moments()
        self._chk(fn(self.ctx, _ptr(buf), n, C.byref(out)))
        return out

    def beam_moments(self, buf, n):
        """phase-space moments of buf = [pos n | vel n | ..] (float32 xyz triplets): a Moments structure with the means, the exact
        extrema, the central second moments, the central fourth moments of every plane (q, p), and from them the rms emittances
        and the halo parameters (nbco_beam_moments).  Two passes over the state, fp64, fixed order; buf is not modified."""
        return self._moments(self.lib.nbco_beam_moments, buf, n)

    def beam_moments_2d(self, buf, n):
        """the same of the 2-D fp64 state [pos n | vel n | ..] of xy pairs (nbco_2d_beam_moments)"""
        return self._moments(self.lib.nbco_2d_beam_moments, buf, n)

    def _hist(self, fn, buf, n, axes, counts):
        if len(axes) == 4 and not hasattr(axes[0], "__len__"):
            axes = [axes]   # one (coord, bins, lo, hi) tuple
        arr = (HistAxis * max(len(axes), 1))(*[HistAxis(int(a[0]), int(a[1]), float(a[2]), float(a[3])) for a in axes])
        if counts is None:
            total = 1
            for a in axes:
                total *= max(int(a[1]), 0)
            if not 1 <= total <= 1 << 24:
                total = 0   # (the library refuses the call; nothing that large is allocated for it)
            counts = self.torch.empty(total + 1, dtype=self.torch.int64, device=buf.device)
        self._chk(fn(self.ctx, _ptr(buf), n, arr, len(axes), _ptr(counts)))
        return counts

    def hist(self, buf, n, axes, counts=None):
        """counts of the particles of buf = [pos n | vel n | ..] over one or two phase-space coordinates (nbco_hist): axes is one
        (coord, bins, lo, hi) tuple or a list of one or two, coord one of Q_X .. Q_VZ.  Returns an int64 device tensor of B + 1
        counts, B = bins0 * bins1 with axis 0 the slow index and the particles outside the window last; `counts` (allocated if
        None) is overwritten.  inside: lo <= q < hi on every axis; bin (int)((q - lo) * (bins / (hi - lo))), clamped to bins - 1."""
        return self._hist(self.lib.nbco_hist, buf, n, axes, counts)

    def hist_2d(self, buf, n, axes, counts=None):
        """the same of the 2-D fp64 state (nbco_2d_hist); the coordinates are Q_X, Q_Y, Q_VX, Q_VY"""
        return self._hist(self.lib.nbco_2d_hist, buf, n, axes, counts)

    def _slice_moments(self, fn, buf, n, axis):
        ax = HistAxis(int(axis[0]), int(axis[1]), float(axis[2]), float(axis[3]))
        records = (Moments * (ax.bins if 1 <= ax.bins <= 65536 else 1))()   # (the library refuses the call; nothing is sized by a bad count)
        outside = C.c_longlong(0)
        self._chk(fn(self.ctx, _ptr(buf), n, C.byref(ax), records, C.byref(outside)))
        return records, outside.value

    def slice_moments(self, buf, n, axis):
        """the moments of beam_moments per slice along one phase-space coordinate (nbco_slice_moments): axis is one
        (coord, bins, lo, hi) tuple, a particle's slice the bin of hist's rule on that coordinate.  Returns (records, n_outside):
        a ctypes array of `bins` Moments, each of its slice's particles alone (an empty slice: n = 0 and zeros), and the number
        of particles outside the window.  fp64, fixed order, a slice's sums independent of the other slices; buf is not modified."""
        return self._slice_moments(self.lib.nbco_slice_moments, buf, n, axis)

    def slice_moments_2d(self, buf, n, axis):
        """the same of the 2-D fp64 state (nbco_2d_slice_moments); the coordinates are Q_X, Q_Y, Q_VX, Q_VY"""
        return self._slice_moments(self.lib.nbco_2d_slice_moments, buf, n, axis)

    # ---- pair statistics -------------------------------------------------------------------------
    def _pair_hist(self, fn, p, n, bins, rmax, counts, nn2):
        if counts is None:
            room = int(bins) if 1 <= int(bins) <= 65536 else 0   # (the library refuses the call; nothing is sized by a bad count)
            counts = self.torch.empty(room + 1, dtype=self.torch.int64, device=p.device)
        elif counts is False:
            counts = None
        self._chk(fn(self.ctx, _ptr(p), n, int(bins), float(rmax), _ptr(counts), _ptr(nn2)))
        return counts

    def pair_hist(self, p, n, bins, rmax, counts=None, nn2=None):
        """pair-distance histogram and nearest neighbours of the n positions p (float32 xyz triplets; the head of a state works), all
        pairs, exact (nbco_pair_hist).  Returns an int64 device tensor of bins + 1 counts of the unordered pairs i < j: bin b holds
        (b w)^2 <= r2 < ((b + 1) w)^2 with w = rmax / bins, in fp64 over the widened coordinates, the last entry the pairs with
        r2 >= rmax^2.  `counts` (allocated if None) is overwritten; counts=False asks for no counts.  nn2: None or a float64 device
        tensor of n that receives, per particle, the smallest r2 to another particle below rmax^2, +inf where there is none.
        p is not modified."""
        return self._pair_hist(self.lib.nbco_pair_hist, p, n, bins, rmax, counts, nn2)

    def pair_hist_tree(self, p, n, bins, rmax, counts=None, nn2=None):
        """the same bytes from a range-limited walk over a kd-tree of its own on a private context (nbco_pair_hist_tree): the cost
        follows the number of pairs near rmax, not n^2; valid in any state of this engine, which it leaves untouched"""
        return self._pair_hist(self.lib.nbco_pair_hist_tree, p, n, bins, rmax, counts, nn2)

    def pair_hist_2d(self, p, n, bins, rmax, counts=None, nn2=None):
        """the exact form for the 2-D fp64 positions (xy pairs; nbco_2d_pair_hist)"""
        return self._pair_hist(self.lib.nbco_2d_pair_hist, p, n, bins, rmax, counts, nn2)

    # ---- bond-orientational order -----------------------------------------------------------------
    def _bond_order(self, fn, p, n, rmax, nb, q, summary):
        room = max(int(n), 0)   # (the library refuses a bad n; nothing is sized by it)
        if nb is None:
            nb = self.torch.empty(room, dtype=self.torch.int32, device=p.device)
        elif nb is False:
            nb = None
        if q is None:
            q = self.torch.empty((room, 2), dtype=self.torch.float64, device=p.device)
        elif q is False:
            q = None
        out = BondSummary() if summary else None
        self._chk(fn(self.ctx, _ptr(p), n, float(rmax), _ptr(nb), _ptr(q), C.byref(out) if summary else None))
        return nb, q, out

    def bond_order(self, p, n, rmax, nb=None, q=None, summary=True):
        """bond-orientational order of the n positions p (float32 xyz triplets; the head of a state works), all pairs, exact
        (nbco_bond_order).  j is a neighbour of i iff 0 < r2 < rmax^2 in fp64 over the widened coordinates.  Returns (nb, q, summary):
        nb an int32 device tensor of n neighbour counts, q a float64 device tensor (n, 2) of the Steinhardt q4 and q6 (0 where
        nb = 0), both in the caller's order, summary a BondSummary (bonds, isolated, nb_max, the means of q over the particles with
        neighbours and the global Q4, Q6).  nb and q are allocated if None and overwritten if given; False asks for none of that
        output, summary=False for no summary (the call then does not synchronise).  p is not modified."""
        return self._bond_order(self.lib.nbco_bond_order, p, n, rmax, nb, q, summary)

    def bond_order_tree(self, p, n, rmax, nb=None, q=None, summary=True):
        """the same from a range-limited walk over a kd-tree of its own on a private context (nbco_bond_order_tree): the cost follows the
        number of bonds, not n^2.  nb is equal integer for integer, q and the summary to rounding (the neighbours are met in another
        order).  Valid in any state of this engine, which it leaves untouched."""
        return self._bond_order(self.lib.nbco_bond_order_tree, p, n, rmax, nb, q, summary)

    def bond_order_2d(self, p, n, rmax, nb=None, q=None, summary=True):
        """the exact form for the 2-D fp64 positions (xy pairs; nbco_2d_bond_order): q holds |psi4| and |psi6|, the hexatic order"""
        return self._bond_order(self.lib.nbco_2d_bond_order, p, n, rmax, nb, q, summary)

    # ---- crystalline particles: bond vector records, solid bonds, averaged order ---------------------
    def _out(self, given, shape, dtype, device):
        """an output by the conventions of _bond_order: None allocates, False asks for none of it"""
        if given is None:
            return self.torch.empty(shape, dtype=dtype, device=device)
        return None if given is False else given

    def _bond_vectors(self, fn, p, n, rmax, nb, vec):
        room = max(int(n), 0)   # (the library refuses a bad n; nothing is sized by it)
        nb = self._out(nb, room, self.torch.int32, p.device)
        vec = self._out(vec, (room, BOND_VEC), self.torch.float64, p.device)
        self._chk(fn(self.ctx, _ptr(p), n, float(rmax), _ptr(nb), _ptr(vec)))
        return nb, vec

    def bond_vectors(self, p, n, rmax, nb=None, vec=None):
        """the bond vector records of the n positions p, all pairs, exact (nbco_bond_vectors): pass 1 of bond_order with the normalised
        S_lm as output.  Returns (nb, vec): nb as bond_order's, vec a float64 device tensor (n, BOND_VEC) -- q^_4m, q^_6m, a_4, a_6 --
        both in the caller's order; allocated if None, overwritten if given, False asks for none of that output."""
        return self._bond_vectors(self.lib.nbco_bond_vectors, p, n, rmax, nb, vec)

    def bond_vectors_tree(self, p, n, rmax, nb=None, vec=None):
        """the same from the kd-tree walk of bond_order_tree on the private context (nbco_bond_vectors_tree)"""
        return self._bond_vectors(self.lib.nbco_bond_vectors_tree, p, n, rmax, nb, vec)

    def _bond_solid(self, fn, p, n, rmax, dmin, xi_min, vec, nb, xi, qbar, summary):
        room = max(int(n), 0)
        nb = self._out(nb, room, self.torch.int32, p.device)
        xi = self._out(xi, room, self.torch.int32, p.device)
        qbar = self._out(qbar, (room, 2), self.torch.float64, p.device)
        out = SolidSummary() if summary else None
        self._chk(fn(self.ctx, _ptr(p), n, float(rmax), _ptr(vec), float(dmin), int(xi_min), _ptr(nb), _ptr(xi), _ptr(qbar), C.byref(out) if summary else None))
        return nb, xi, qbar, out

    def bond_solid(self, p, n, rmax, dmin, xi_min, vec=None, nb=None, xi=None, qbar=None, summary=True):
        """which of the n positions p are crystalline, all pairs, exact (nbco_bond_solid): per particle the number xi of SOLID bonds --
        neighbours j with d6(i, j) > dmin, d6 the dot product of the two q^_6 vectors -- and the neighbour-averaged q-bar_4, q-bar_6.
        vec: the records of bond_vectors (read only), or None: the call forms them itself and returns the same bytes.  Returns
        (nb, xi, qbar, summary): int32 (n), int32 (n), float64 (n, 2) device tensors in the caller's order and a SolidSummary (n_solid =
        #{xi >= xi_min}, solid_bonds, xi_max, the means of q-bar over the particles with neighbours).  Outputs are allocated if None,
        overwritten if given; False asks for none of that output, summary=False for no summary (the call then does not synchronise)."""
        return self._bond_solid(self.lib.nbco_bond_solid, p, n, rmax, dmin, xi_min, vec, nb, xi, qbar, summary)

    def bond_solid_tree(self, p, n, rmax, dmin, xi_min, vec=None, nb=None, xi=None, qbar=None, summary=True):
        """the same from a kd-tree of its own on the private context (nbco_bond_solid_tree); with vec=None one tree and two walks.  For
        the same records nb, xi and the summary's integers are equal integer for integer, q-bar to rounding."""
        return self._bond_solid(self.lib.nbco_bond_solid_tree, p, n, rmax, dmin, xi_min, vec, nb, xi, qbar, summary)

    # ---- static structure factor -------------------------------------------------------------------
    def _structure_factor(self, fn, dim, p, n, h, kstep, rho, count):
        g = SkGrid()
        for a in range(dim):
            g.h[a] = int(h[a])
            g.kstep[a] = float(kstep[a])
        if rho is None:
            ok = all(0 <= int(h[a]) <= 64 for a in range(dim))   # (the library refuses the call; nothing is sized by a bad h)
            K = (int(h[0]) + 1) * (2 * int(h[1]) + 1) * (2 * int(h[2]) + 1 if dim == 3 else 1) if ok else 0
            rho = self.torch.empty(K, dtype=self.torch.complex128, device=p.device)
        used = C.c_longlong(0)
        self._chk(fn(self.ctx, _ptr(p), n, C.byref(g), _ptr(rho), C.byref(used) if count else None))
        return rho, (used.value if count else None)

    def structure_factor(self, p, n, h, kstep, rho=None, count=True):
        """rho_k = sum_j exp(i k . x_j) of the n positions p (float32 xyz triplets; the head of a state works) on the grid
        k = (ix kstep[0], iy kstep[1], iz kstep[2]), ix = 0..h[0], iy = -h[1]..h[1], iz = -h[2]..h[2] (nbco_structure_factor).
        Returns (rho, n_used): rho a complex128 device tensor of K = (h[0]+1)(2 h[1]+1)(2 h[2]+1) values at index
        (ix (2 h[1]+1) + iy + h[1]) (2 h[2]+1) + iz + h[2] (allocated if None, overwritten if given), n_used the number of particles
        that counted (those with finite coordinates); rho at k = 0 is exactly n_used.  count=False returns n_used = None and does
        not synchronise.  S(k) = |rho|^2 / n_used is the caller's.  p is not modified."""
        return self._structure_factor(self.lib.nbco_structure_factor, 3, p, n, h, kstep, rho, count)

    def structure_factor_2d(self, p, n, h, kstep, rho=None, count=True):
        """the same for the 2-D fp64 positions (xy pairs; nbco_2d_structure_factor): K = (h[0]+1)(2 h[1]+1), index ix (2 h[1]+1) + iy + h[1]"""
        return self._structure_factor(self.lib.nbco_2d_structure_factor, 2, p, n, h, kstep, rho, count)

    # ---- tracked trajectories and their time correlations ------------------------------------------
    def traj_record(self, buf, n, traj, frame, stride=1, ids=None):
        """writes frame `frame` of the trajectory buffer traj (a float32 device tensor rows x frames_cap x 6: x y z vx vy vz of the
        particle with number row * stride) from the state buf = [pos n | vel n ..] (nbco_traj_record): the frame is first filled
        with NaN, then every state row whose particle number p has p % stride == 0 and p // stride < rows is copied with its bits.
        p is ids[i] (an int32 device tensor) if given, else the engine's order map where tracking is live (track_order = 1 and
        unsort = 0 evaluations of these n particles), else the row.  A lost particle's later frames stay NaN.  The state and the
        engine are not touched; enqueued on the engine's stream."""
        rows, cap = int(traj.shape[0]), int(traj.shape[1])
        self._chk(self.lib.nbco_traj_record(self.ctx, _ptr(buf), n, _ptr(ids), _ptr(traj), rows, cap, int(frame), int(stride)))

    def time_corr(self, traj, rows, frames, lags, out=None):
        """the raw time-correlation sums of the first `rows` rows and `frames` frames of traj for the lags 0 .. lags - 1
        (nbco_time_corr; 1 <= lags <= frames <= traj.shape[1], frames <= 2048): a float64 device tensor lags x 8 (allocated if None,
        overwritten if given) whose rows are nbco_corr_lag records -- dx2[3], r4, vv[3] and, in the last 8 bytes, the integer
        pairs: out.cpu().numpy().view(CORR_LAG) reads them, time_corr_derive(out) gives msd, alpha2 and vacf.  A (row, t, lag) counts
        only if both frames are finite.  The same bytes on every call.  traj is not modified."""
        if out is None:
            out = self.torch.empty((max(int(lags), 0), 8), dtype=self.torch.float64, device=traj.device)
        self._chk(self.lib.nbco_time_corr(self.ctx, _ptr(traj), int(rows), int(traj.shape[1]), int(frames), int(lags), _ptr(out)))
        return out

    # ---- collective modes ----------------------------------------------------------------------------
    def modes_record(self, buf, n, h, kstep, series=None, frames_cap=1, frame=0, count=True):
        """the mode records {rho, jx, jy, jz} (complex: eight doubles) of the state buf = [pos n | vel n ..] on the grid of
        structure_factor, written to frame `frame` of series, a float64 device tensor K x frames_cap x 8 (nbco_modes_record;
        allocated if None -- the other frames then hold whatever the allocation held -- and only that frame overwritten if given,
        its frames_cap then taken from the tensor).  Returns (series, n_used): n_used the number of particles that counted (finite
        position and velocity); rho at k = 0 is exactly (n_used, 0).  count=False returns n_used = None and does not synchronise.
        The state and the engine are not touched."""
        if series is None:
            series = self.torch.empty((_sk_count(h), max(int(frames_cap), 0), 8), dtype=self.torch.float64, device=buf.device)
        else:
            frames_cap = int(series.shape[1])
        used = C.c_longlong(0)
        g = _sk_grid(h, kstep)
        self._chk(self.lib.nbco_modes_record(self.ctx, _ptr(buf), n, C.byref(g), _ptr(series), int(frames_cap), int(frame), C.byref(used) if count else None))
        return series, (used.value if count else None)

    def mode_corr(self, series, h, kstep, frames, lags, out=None):
        """the raw time-correlation sums of the first `frames` frames of every k of series (as modes_record fills it) for the lags
        0 .. lags - 1 (nbco_mode_corr; 1 <= lags <= frames <= series.shape[1], frames <= 1024): a float64 device tensor
        K x lags x 8 (allocated if None, overwritten if given) whose rows are nbco_mode_lag records -- rr, ll, jj, s0[2], s1[2] and,
        in the last 8 bytes, the integer pairs: out.cpu().numpy().view(MODE_LAG) reads them, mode_corr_derive(out, h, kstep, n)
        gives F, F_c, C_L and C_T.  The bytes are those of mode_corr_ref for the same series.  series is not modified."""
        if out is None:
            out = self.torch.empty((_sk_count(h), max(int(lags), 0), 8), dtype=self.torch.float64, device=series.device)
        g = _sk_grid(h, kstep)
        self._chk(self.lib.nbco_mode_corr(self.ctx, _ptr(series), C.byref(g), int(series.shape[1]), int(frames), int(lags), _ptr(out)))
        return out

    # ---- aperture ---------------------------------------------------------------------------------
    @staticmethod
    def _aperture(dim, shape, half, centre):
        half = [float(h) for h in half]
        centre = [0.0] * dim if centre is None else [float(v) for v in centre]
        if len(half) != dim or len(centre) != dim:
            raise EngineError("aperture: half and centre take %d values" % dim)
        pad = [0.0] * (3 - dim)
        return Aperture(int(shape), (C.c_double * 3)(*(centre + pad)), (C.c_double * 3)(*(half + pad)))

    def _aperture_count(self, fn, dim, p, n, shape, half, centre):
        ap, lost = self._aperture(dim, shape, half, centre), C.c_longlong(-1)
        self._chk(fn(self.ctx, _ptr(p), n, C.byref(ap), C.byref(lost)))
        return lost.value

    def _aperture_apply(self, fn, dim, buf, n, shape, half, centre, lost, lost_row):
        ap, kept = self._aperture(dim, shape, half, centre), C.c_longlong(-1)
        room = [t.numel() // w for t, w in ((lost, 2 * dim), (lost_row, 1)) if t is not None]

        def where(t):   # (torch gives an empty view the address 0, which the library reads as "no output": a record without room is still one)
            return None if t is None else C.c_void_p(t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size())
        rc = fn(self.ctx, _ptr(buf), n, C.byref(ap), C.byref(kept), where(lost), where(lost_row), min(room) if room else 0)
        if rc != 0:
            e = EngineError("nbco status %d: %s" % (rc, self.lib.nbco_last_error(self.ctx).decode()), status=rc)
            e.n_kept = kept.value if rc == ERR_CAPACITY else None   # (what the record of a second call is sized from)
            raise e
        return kept.value

    def aperture_count(self, p, n, shape, half, centre=None):
        """number of the n positions p (float32 xyz triplets) outside the aperture (nbco_aperture_count): shape AP_ELLIPSOID or AP_BOX,
        half the three half axes (float("inf") opens an axis), centre the three coordinates of its centre (default 0).  The rule is
        that of include/nbco.h, in fp64.  p and the engine's state are not touched.  Synchronises."""
        return self._aperture_count(self.lib.nbco_aperture_count, 3, p, n, shape, half, centre)

    def aperture(self, buf, n, shape, half, centre=None, lost=None, lost_row=None):
        """drops the particles outside the aperture from the state buf = [pos n | vel n | acc n] (float32) and returns n_kept: buf then
        holds [pos n_kept | vel n_kept | acc n_kept] at its head, the kept particles in their order (nbco_aperture_apply).
        lost: None or a float32 device tensor that receives x y z vx vy vz per lost particle, in state order; lost_row: None or an
        int32 device tensor that receives their rows in buf before the call.  The capacity of the record is taken from the tensors;
        when more are lost, nothing is changed and the EngineError (status ERR_CAPACITY) carries n_kept.  A call that loses
        nobody changes nothing at all; one that loses somebody drops the tree: energy_fmm / energy_kd / probe_kd must follow the next
        evaluation.  Synchronises."""
        return self._aperture_apply(self.lib.nbco_aperture_apply, 3, buf, n, shape, half, centre, lost, lost_row)

    def aperture_count_2d(self, p, n, shape, half, centre=None):
        """the same of the 2-D fp64 positions (xy pairs; nbco_2d_aperture_count); half and centre take two values"""
        return self._aperture_count(self.lib.nbco_2d_aperture_count, 2, p, n, shape, half, centre)

    def aperture_2d(self, buf, n, shape, half, centre=None, lost=None, lost_row=None):
        """the same of the 2-D fp64 state (nbco_2d_aperture_apply); a loss record is x y vx vy, float64"""
        return self._aperture_apply(self.lib.nbco_2d_aperture_apply, 2, buf, n, shape, half, centre, lost, lost_row)

    # ---- multi-GPU kd-domain sharding (see dist.py for the orchestration) ---------------------------
    def dist_layout(self, n_global, world, rank):
        lay = DistLayout()
        self._chk(self.lib.nbco_dist_layout_query(self.ctx, n_global, world, rank, C.byref(lay)))
        return lay

    def dist_partition(self, state_all, n_global, world, rank, state_local):
        self._chk(self.lib.nbco_dist_partition(self.ctx, _ptr(state_all), n_global, world, rank, _ptr(state_local)))

    def dist_local(self, buf_local, n_local, nodes_send, pos_send):
        self._chk(self.lib.nbco_dist_local(self.ctx, _ptr(buf_local), n_local, _ptr(nodes_send), _ptr(pos_send)))

    def dist_local_build(self, buf_local, n_local, pos_send):
        self._chk(self.lib.nbco_dist_local_build(self.ctx, _ptr(buf_local), n_local, _ptr(pos_send)))

    def dist_local_upward(self, buf_local, n_local, nodes_send):
        self._chk(self.lib.nbco_dist_local_upward(self.ctx, _ptr(buf_local), n_local, _ptr(nodes_send)))

    # the same evaluation with the node block in two all-gathers (traversal records first, multipoles later)
    def dist_local_geom(self, buf_local, n_local, pos_send, csz_send):
        self._chk(self.lib.nbco_dist_local_geom(self.ctx, _ptr(buf_local), n_local, _ptr(pos_send), _ptr(csz_send)))

    def dist_local_mpole(self, buf_local, n_local, mpole_send):
        self._chk(self.lib.nbco_dist_local_mpole(self.ctx, _ptr(buf_local), n_local, _ptr(mpole_send)))

    def dist_finish_traverse(self, csz_all, pos_all):
        self._chk(self.lib.nbco_dist_finish_traverse(self.ctx, _ptr(csz_all), _ptr(pos_all)))

    def dist_finish_rest(self, mpole_all, buf_local, a_local, param=None):
        self._chk(self.lib.nbco_dist_finish_rest(self.ctx, _ptr(mpole_all), _ptr(buf_local), _ptr(a_local), _ptr(param)))

    # the re-partition without gathering the state (include/nbco.h: nbco_dist_repartition_*)
    def dist_repartition_workspace(self, n_global, world):
        b = C.c_longlong()
        self._chk(self.lib.nbco_dist_repartition_workspace(self.ctx, n_global, world, C.byref(b)))
        return int(b.value)

    def dist_repartition_begin(self, state_local, n_global, world, rank, work):
        st = DistStep()
        self._chk(self.lib.nbco_dist_repartition_begin(self.ctx, _ptr(state_local), n_global, world, rank, _ptr(work), work.numel() * work.element_size(),
                                                       C.byref(st)))
        return st

    def dist_repartition_next(self):
        st = DistStep()
        self._chk(self.lib.nbco_dist_repartition_next(self.ctx, C.byref(st)))
        return st

    # the same evaluation with the LET exchange (include/nbco.h: nbco_dist_let_*)
    def dist_let_local_geom(self, buf_local, n_local, csz_send):
        self._chk(self.lib.nbco_dist_let_local_geom(self.ctx, _ptr(buf_local), n_local, _ptr(csz_send)))

    def dist_let_local_mpole(self, buf_local, n_local):
        self._chk(self.lib.nbco_dist_let_local_mpole(self.ctx, _ptr(buf_local), n_local))

    def dist_let_select(self, csz_all, counts_send):
        self._chk(self.lib.nbco_dist_let_select(self.ctx, _ptr(csz_all), _ptr(counts_send)))

    def dist_let_pack(self, counts_all_host, pos_send, mpole_send):
        self._chk(self.lib.nbco_dist_let_pack(self.ctx, _ptr(counts_all_host), _ptr(pos_send), _ptr(mpole_send)))

    def dist_let_finish(self, counts_all_host, pos_recv, mpole_recv, buf_local, a_local, param=None):
        self._chk(self.lib.nbco_dist_let_finish(self.ctx, _ptr(counts_all_host), _ptr(pos_recv), _ptr(mpole_recv), _ptr(buf_local), _ptr(a_local),
                                                _ptr(param)))

    def dist_turnaround(self, buf_local, n_local, param, dt, scale=1.0, elastic=True):
        """one pass between two force evaluations of a sharded leapfrog run (nbco_dist_turnaround)"""
        self._chk(self.lib.nbco_dist_turnaround(self.ctx, _ptr(buf_local), n_local, _ptr(param), dt, scale, int(elastic)))

    def dist_let_check(self):
        self._chk(self.lib.nbco_dist_let_check(self.ctx))

    # the exchange with segments sized ahead of the counts (nbco_dist_let_pack_capped): caps_* are host int64 tensors of 2 world values
    def dist_let_pack_capped(self, caps_out_host, pos_send, mpole_send):
        self._chk(self.lib.nbco_dist_let_pack_capped(self.ctx, _ptr(caps_out_host), _ptr(pos_send), _ptr(mpole_send)))

    def dist_let_finish_capped(self, caps_in_host, pos_recv, mpole_recv, buf_local, a_local, param=None):
        self._chk(self.lib.nbco_dist_let_finish_capped(self.ctx, _ptr(caps_in_host), _ptr(pos_recv), _ptr(mpole_recv), _ptr(buf_local), _ptr(a_local),
                                                       _ptr(param)))

    def dist_let_settle(self, ok):
        self._chk(self.lib.nbco_dist_let_settle(self.ctx, int(bool(ok))))

    def aux_stream(self):
        """raw hipStream_t of the context's second stream (see nbco_aux_stream)"""
        out = C.c_void_p()
        self._chk(self.lib.nbco_aux_stream(self.ctx, C.byref(out)))
        return out.value or 0

    def dist_finish(self, nodes_all, pos_all, buf_local, a_local, param=None):
        self._chk(self.lib.nbco_dist_finish(self.ctx, _ptr(nodes_all), _ptr(pos_all), _ptr(buf_local), _ptr(a_local), _ptr(param)))

    # ---- kd-tree introspection ------------------------------------------------------------------
    def kd_info(self):
        info = KdInfo()
        self._chk(self.lib.nbco_kd_get_info(self.ctx, C.byref(info)))
        return info

    def kd_array(self, name):
        import numpy as np
        info = self.kd_info()
        p = info.order
        offM, offL = p * (p + 1) * (p + 2) // 6, (p + 1) ** 2
        real = np.float64 if info.real_bytes == 8 else np.float32      # doubles after an evaluation with far_fp64
        shapes = {"mult": ((info.ntot,), np.int32), "index": ((info.ntot,), np.int32), "splitdim": ((info.ntot,), np.int32),
                  "center": ((info.ntot, 3), np.float32), "lbound": ((info.ntot, 3), np.float32),
                  "rbound": ((info.ntot, 3), np.float32), "mpole": ((info.ntot, offM), real),
                  "local": ((info.ntot, offL), real), "p2p": ((info.p2p_pairs, 2), np.int32),
                  "m2l": ((info.m2l_pairs, 2), np.int32), "unsort": ((info.n,), np.int32), "order": ((info.n,), np.int32)}
        shape, dt = shapes[name]
        out = np.empty(shape, dtype=dt)
        if out.size:
            self._chk(self.lib.nbco_kd_copy(self.ctx, KD_FIELDS[name], out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    # ---- octree introspection -----------------------------------------------------------------------
    def oct_info(self):
        info = OctInfo()
        self._chk(self.lib.nbco_oct_get_info(self.ctx, C.byref(info)))
        return info

    def oct_array(self, name):
        import numpy as np
        info = self.oct_info()
        off = (info.order + 1) ** 2
        real = np.float64 if info.real_bytes == 8 else np.float32
        shapes = {"mult": ((info.ntot,), np.int32), "index": ((info.ntot,), np.int32), "center4": ((info.ntot, 4), np.float32),
                  "mpole": ((info.ntot, info.mpole_reals), real), "local": ((info.ntot, off), real),
                  "keys": ((info.n,), np.uint32), "perm": ((info.n,), np.uint32)}
        shape, dt = shapes[name]
        out = np.empty(shape, dtype=dt)
        self._chk(self.lib.nbco_oct_copy(self.ctx, OCT_FIELDS[name], out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    # ---- checked build (libnbco_hip_checked.so, selected with NBCO_LIB) ------------------------------------
    def violations(self):
        """per-site counts of list-derived indices that failed their range check on the device (checked build only)"""
        out = (C.c_longlong * 8)()
        self._chk(self.lib.nbco_debug_violations(self.ctx, out))
        return list(out)

    # ---- profiling ------------------------------------------------------------------------------
    def profile(self, phases=True):
        """phases: True = all, False = off, or an iterable of phase names (see PHASES)."""
        if phases is True:
            mask = -1
        elif not phases:
            mask = 0
        else:
            mask = 0
            for name in phases:
                mask |= 1 << PHASES.index(name)
        self._chk(self.lib.nbco_profile_enable(self.ctx, mask))

    def profile_reset(self):
        self._chk(self.lib.nbco_profile_reset(self.ctx))

    def profile_get(self):
        out = {}
        for i, name in enumerate(PHASES):
            ms, cnt = C.c_double(), C.c_longlong()
            self._chk(self.lib.nbco_profile_get(self.ctx, i, C.byref(ms), C.byref(cnt)))
            out[name] = (ms.value, cnt.value)
        return out
