"""ctypes mirror of include/mcs.h (the C ABI of the transport path).

The structures here are laid out exactly as in the header; `tests/test_abi.py`
checks sizes, the tally layout and that the shared library exports every
declared symbol.
"""
from __future__ import annotations

import ctypes as ct
import os
from typing import Dict

import numpy as np

from .constants import PSD_MAX, NA_C

MCS_ABI_VERSION = 3

c_double_p = ct.POINTER(ct.c_double)
c_int64_p = ct.POINTER(ct.c_int64)
c_uint8_p = ct.POINTER(ct.c_uint8)
c_int32_p = ct.POINTER(ct.c_int32)


class McsParams(ct.Structure):
    """`mcs_params`: the scalars/flags of src/main_loops.jl:236-264."""
    _fields_ = [
        ("abi_version", ct.c_int32),
        ("n_ions", ct.c_int32), ("n_grid", ct.c_int32), ("n_itrs", ct.c_int32),
        ("n_pts_max", ct.c_int64),
        ("i_grid_feb", ct.c_int32), ("i_shock", ct.c_int32),
        ("num_psd_mom_bins", ct.c_int32), ("num_psd_tht_bins", ct.c_int32),
        ("psd_bins_per_dec_mom", ct.c_int32), ("psd_bins_per_dec_tht", ct.c_int32),
        ("psd_cos_fine", ct.c_double), ("psd_dcos", ct.c_double), ("psd_tht_min", ct.c_double),
        ("psd_mom_min", ct.c_double),
        ("gam0", ct.c_double), ("beta0", ct.c_double), ("u0", ct.c_double), ("u2", ct.c_double),
        ("bmag2", ct.c_double),
        ("pe_crit", ct.c_double), ("game_crit", ct.c_double), ("eta_mfp", ct.c_double),
        ("energy_transfer_frac", ct.c_double),
        ("feb_upstream", ct.c_double), ("feb_downstream", ct.c_double), ("x_grid_stop", ct.c_double),
        ("B_CMBz", ct.c_double), ("age_max", ct.c_double),
        ("xn_per_fine", ct.c_double), ("xn_per_coarse", ct.c_double),
        ("use_custom_epsB", ct.c_int32), ("do_rad_losses", ct.c_int32), ("do_retro", ct.c_int32),
        ("do_tcuts", ct.c_int32),
        ("dont_DSA", ct.c_int32), ("dont_scatter", ct.c_int32), ("use_custom_frg", ct.c_int32),
        ("track_thermal", ct.c_int32),
        ("state_fp32", ct.c_int32),
    ]


class McsSoa(ct.Structure):
    """`mcs_soa`: host struct-of-arrays population (Float64 / Int / Bool as in Julia)."""
    _fields_ = [
        ("weight", c_double_p), ("ptot_pf", c_double_p), ("pb_pf", c_double_p), ("x_PT_cm", c_double_p),
        ("xn_per", c_double_p), ("prp_x_cm", c_double_p), ("acctime_sec", c_double_p), ("phi_rad", c_double_p),
        ("grid", c_int64_p), ("tcut", c_int64_p),
        ("downstream", c_uint8_p), ("inj", c_uint8_p),
    ]


class McsConsumerIn(ct.Structure):
    """`mcs_consumer_in`: host tables for the tally consumers (include/mcs.h)."""
    _fields_ = [
        ("mom_log_cgs", c_double_p), ("mom_edge_cgs", c_double_p), ("cos_edge", c_double_p),
        ("cos_center", c_double_p), ("pt_center", c_double_p), ("zone_pop", c_double_p),
        ("density_loc", c_double_p), ("cold_pressure", c_double_p),
        ("rest_energy", ct.c_double), ("mc", ct.c_double), ("n0", ct.c_double), ("gam0", ct.c_double),
        ("therm_from_hist", ct.c_int),
    ]


class McsOptionDesc(ct.Structure):
    """`mcs_option_desc`: one row of the library's option table (include/mcs.h, enum mcs_option)."""
    _fields_ = [
        ("key", ct.c_int32), ("when", ct.c_int32), ("applies", ct.c_int32), ("reserved", ct.c_int32),
        ("min", ct.c_int64), ("max", ct.c_int64), ("dflt", ct.c_int64),
        ("name", ct.c_char_p), ("env", ct.c_char_p),
    ]


class McsEnsLayout(ct.Structure):
    """`mcs_ens_layout`: offsets and lengths of the parts of the two sample vectors of the ensemble statistics (include/mcs.h)."""
    _fields_ = [(name, ct.c_int64) for name in (
        "sp_tallies", "sp_tallies_n", "sp_recv_pool", "sp_recv_pool_n", "sp_num_crossings", "sp_num_crossings_n",
        "sp_psd_mom", "sp_psd_tht", "sp_therm_sf_mom", "sp_therm_sf_tht", "sp_therm_pf_mom", "sp_therm_pf_tht",
        "sp_marg_mom_n", "sp_marg_tht_n", "sp_total",
        "it_sums", "it_sums_n", "it_scalars", "it_scalars_n", "it_total",
        "tally_sp_first", "tally_it_first", "tally_recv_pool", "tally_scalars")]


class McsEnsProductsLayout(ct.Structure):
    """`mcs_ens_products_layout`: offsets and lengths of the nine parts of a products sample (include/mcs.h, "products sample")."""
    _fields_ = [(name, ct.c_int64) for name in (
        "dNdp_sf", "dNdp_pf", "dNdp_isf", "dNdp_n", "P_psd_par", "P_psd_perp", "energy_density_psd",
        "slope_sf", "slope_pf", "slope_isf", "zone_n", "total")]


ENS_PRODUCTS_BIT = 1 << 30      # MCS_ENS_PRODUCTS(s) = s | ENS_PRODUCTS_BIT


class McsEnsPhotonsLayout(ct.Structure):
    """`mcs_ens_photons_layout`: offsets and row lengths of the four sections of a photons sample (include/mcs.h, "photons sample")."""
    _fields_ = [(name, ct.c_int64) for name in ("synch", "ic", "pion", "total_section", "n_synch", "n_ic", "n_pion", "n_pts", "rows", "total")]


class McsEnsEscapeLayout(ct.Structure):
    """`mcs_ens_escape_layout`: offsets of the three parts of an escape sample and the length of a dN/dp row (include/mcs.h,
    "escape sample")."""
    _fields_ = [(name, ct.c_int64) for name in ("dNdp", "number", "slope", "row_n", "total")]


class McsEnsAnglesLayout(ct.Structure):
    """`mcs_ens_angles_layout`: offsets of the four parts of an angles sample, the length of a dist row and the number of rows
    (include/mcs.h, "angles sample")."""
    _fields_ = [(name, ct.c_int64) for name in ("dist", "number", "mean_mu", "mean_mu2", "row_n", "rows", "total")]


class McsTcutLayout(ct.Structure):
    """`mcs_tcut_layout` (= `mcs_ens_tcuts_layout`): offsets of the six parts of a time-cut result, the length of a spectrum row and the
    number of cuts (include/mcs.h, mcs_tcut_spectra and "tcuts sample")."""
    _fields_ = [(name, ct.c_int64) for name in ("spectrum", "weight", "number", "mean_log_p", "quantile", "index", "row_n", "n_tcuts", "total")]


class McsProfileIn(ct.Structure):
    """`mcs_profile_in`: what the host hands to the profile update (include/mcs.h, mcs_profile_update); the fields up to i_trans are
    the settings an ensemble keeps of its first profile sample."""
    _fields_ = [(name, ct.c_double) for name in ("F_px_upstream", "F_energy_upstream", "P0", "rho0", "n0_aa", "r_comp", "r_RH", "u2", "beta2",
                                                 "gam2", "SMMOE", "SMPFP", "w")] + \
               [("i_trans", ct.c_int32), ("n_hist", ct.c_int32), ("hist_q_px", ct.c_double * 3), ("hist_q_en", ct.c_double * 3)] + \
               [(name, ct.POINTER(ct.c_double)) for name in ("pxx_EM", "en_EM", "atan_x")]


class McsProfileLayout(ct.Structure):
    """`mcs_profile_layout` (= `mcs_ens_profile_layout`): offsets of the ten rows and of the scalars of a profile update, the length of a
    row and the number of scalars (include/mcs.h, mcs_profile_update and "profile sample")."""
    _fields_ = [(name, ct.c_int64) for name in ("flux_px", "flux_en", "gamma_ad", "p_flux", "p_used", "ux_px", "ux_en", "ux_pred", "ux_next",
                                                "shift", "scalars", "row_n", "n_scalars", "total")]


class McsDetectorLayout(ct.Structure):
    """`mcs_detector_layout` (= `mcs_ens_detectors_layout`): offsets of the seven parts of a detector result, the length of a row and the
    number of detectors (include/mcs.h, mcs_detector_spectra and "detectors sample")."""
    _fields_ = [(name, ct.c_int64) for name in ("spectrum", "dndp", "number", "mean_log_p", "quantile", "slope", "gradient", "row_n", "n_det", "total")]


TCUT_Q = (0.5, 0.9, 0.99)       # MCS_TCUT_Q
ENS_DETECTORS_BIT = 1 << 23     # MCS_ENS_DETECTORS(s) = s | ENS_DETECTORS_BIT
ENS_PROFILE = 1 << 24           # MCS_ENS_PROFILE: the profile slot, one per accumulator
ENS_ESCAPE_BIT = 1 << 27        # MCS_ENS_ESCAPE(s) = s | ENS_ESCAPE_BIT
ENS_ANGLES_BIT = 1 << 26        # MCS_ENS_ANGLES(s) = s | ENS_ANGLES_BIT
ENS_TCUTS_BIT = 1 << 25         # MCS_ENS_TCUTS(s) = s | ENS_TCUTS_BIT
ENS_PHOTONS_BIT = 1 << 29       # MCS_ENS_PHOTONS(s) = s | ENS_PHOTONS_BIT
ENS_PHOTONS_ALL = 1 << 28       # MCS_ENS_PHOTONS_ALL: the source slot, one per accumulator


class McsEnsRange(ct.Structure):
    """`mcs_ens_range`: a word range of a slot's sample vector, with the floor and the tolerance of its summary (include/mcs.h)."""
    _fields_ = [("first", ct.c_int64), ("count", ct.c_int64), ("floor_frac", ct.c_double), ("tol", ct.c_double)]


class McsEnsSummary(ct.Structure):
    """`mcs_ens_summary`: what `mcs_ens_summarize` says about one range (include/mcs.h)."""
    _fields_ = [(name, ct.c_double) for name in ("amax", "max_rel", "sum_se", "sum_abs_mean", "sum_rel2")] + \
               [(name, ct.c_int64) for name in ("n_selected", "n_over", "n_nonfinite", "argmax")]


class McsEnsCmpRange(ct.Structure):
    """`mcs_ens_cmp_range`: a word range of the two slots of a comparison, with its floor and its |z| cut (include/mcs.h)."""
    _fields_ = [("first", ct.c_int64), ("count", ct.c_int64), ("floor_frac", ct.c_double), ("zcut", ct.c_double)]


class McsEnsDifference(ct.Structure):
    """`mcs_ens_difference`: what `mcs_ens_compare` says about one range (include/mcs.h)."""
    _fields_ = [(name, ct.c_double) for name in ("amax", "max_abs_z", "sum_z", "sum_abs_z", "sum_z2", "sum_abs_diff", "sum_scale")] + \
               [(name, ct.c_int64) for name in ("n_selected", "n_over", "n_nonfinite", "n_degenerate", "argmax")]


class McsPcutEval(ct.Structure):
    """`mcs_pcut_eval`: the inputs and outputs of `mcs_eval_pcut_split` (include/mcs.h, test hooks)."""
    _fields_ = [(name, ct.c_int32) for name in ("form", "match", "export_mode", "reserved")] + \
               [(name, ct.c_int64) for name in ("n", "cap_n", "src_fill", "i_mult", "n_target", "n_main_next", "guard", "out_cap",
                                                "exp_cap", "exp_first", "exp_stride")] + \
               [("ctr_work", ct.c_uint64), ("ctr_saved", ct.c_uint64),
                ("l_save", c_uint8_p), ("saved", ct.POINTER(McsSoa)), ("exp_gin", c_int64_p),
                ("src", c_int64_p), ("out_f64", c_double_p), ("out_meta", ct.POINTER(ct.c_uint32)),
                ("exp_gidx", c_int64_p), ("exp_f64", c_double_p), ("exp_meta", ct.POINTER(ct.c_uint32))] + \
               [(name, ct.c_uint64) for name in ("scan_total", "ctr_work_after", "ctr_saved_after", "mismatch")] + \
               [("pd", ct.c_int64 * 4), ("pd_next", ct.c_int64 * 4)]


# enum mcs_option_when / mcs_option_applies
OPTION_WHEN = ("between launches", "before the first pipelined run", "creation only")
OPTION_APPLIES = ("any", "fp64 state when > 0", "fp32 state")

F64_FIELDS = ("weight", "ptot_pf", "pb_pf", "x_PT_cm", "xn_per", "prp_x_cm", "acctime_sec", "phi_rad")
I64_FIELDS = ("grid", "tcut")
U8_FIELDS = ("downstream", "inj")


class Population:
    """Numpy struct-of-arrays particle population; the `*_new` / `*_saved`
    arrays of src/MonteCarloScattering.jl:556-585."""

    def __init__(self, n: int):
        self.n = int(n)
        for f in F64_FIELDS:
            setattr(self, f, np.zeros(self.n, dtype=np.float64))
        for f in I64_FIELDS:
            setattr(self, f, np.zeros(self.n, dtype=np.int64))
        for f in U8_FIELDS:
            setattr(self, f, np.zeros(self.n, dtype=np.uint8))

    def soa(self) -> McsSoa:
        s = McsSoa()
        for f in F64_FIELDS:
            setattr(s, f, getattr(self, f).ctypes.data_as(c_double_p))
        for f in I64_FIELDS:
            setattr(s, f, getattr(self, f).ctypes.data_as(c_int64_p))
        for f in U8_FIELDS:
            setattr(s, f, getattr(self, f).ctypes.data_as(c_uint8_p))
        return s

    def fields(self):
        return F64_FIELDS + I64_FIELDS + U8_FIELDS

    def take(self, idx) -> "Population":
        out = Population(len(idx))
        for f in self.fields():
            getattr(out, f)[:] = getattr(self, f)[idx]
        return out

    def slice(self, a: int, b: int) -> "Population":
        return self.take(np.arange(a, b))

    @staticmethod
    def concat(pops) -> "Population":
        out = Population(sum(p.n for p in pops))
        for f in out.fields():
            if pops:
                getattr(out, f)[:] = np.concatenate([getattr(p, f) for p in pops])
        return out


# int64 tally slots after the n_grid num_crossings entries (enum in mcs.h)
IC = {name: i for i, name in enumerate([
    "STEPS_HELIX", "STEPS_RETRO", "HELIX_CAP", "PPERP_CLAMP", "PSP_CLAMP", "MOMBIN_CLAMP",
    "REASON0", "REASON1", "REASON2", "REASON3", "REASON4", "TCUT_OVERRUN", "RNG_DRAWS", "ZONE_FAIL", "RETRO_CAP"])}
IC_COUNT = len(IC)

FN = {name: i for i, name in enumerate(
    ["sin", "cos", "asin", "acos", "atan2", "log10", "mod2pi", "sqrt", "div", "hypot1", "uniform",
     # the transport kernel's own forms, evaluated inside its translation unit (enum mcs_fn, include/mcs.h)
     "sqrt_fast", "sqrt_nn", "sqrt_nn_k", "hypot1_hot", "fdiv", "div_r", "div_r2", "sin_t", "cos_t", "asin_t", "asin_tk",
     "mod2pi_k"])}


class Layout:
    """Python mirror of `mcs_tally_layout` (include/mcs.h): offsets, in doubles,
    of every fp64 tally inside the flat buffer."""

    def __init__(self, P: McsParams):
        nm, nt, ng = P.num_psd_mom_bins + 2, P.num_psd_tht_bins + 2, P.n_grid
        pm = PSD_MAX + 1
        self.shapes: Dict[str, tuple] = {}
        self.offsets: Dict[str, int] = {}
        o = 0
        for name, shape in [
            ("psd", (ng, nt, nm)), ("therm_sf", (ng, nt, nm)), ("therm_pf", (ng, nt, nm)),
            ("esc_psd_up", (pm, pm)), ("esc_psd_down", (pm, pm)),
            ("pxx_flux", (ng,)), ("pxz_flux", (ng,)), ("energy_flux", (ng,)),
            ("esc_flux", (P.n_ions,)),
            ("px_esc_feb", (P.n_itrs, P.n_ions)), ("energy_esc_feb", (P.n_itrs, P.n_ions)),
            ("esc_energy_eff", (P.n_ions, pm)), ("esc_num_eff", (P.n_ions, pm)),
            ("weight_coupled", (P.n_ions, NA_C)), ("spectra_coupled", (P.n_ions, NA_C, pm)),
            ("spectra_sf", (ng, pm)), ("spectra_pf", (ng, pm)),
            ("energy_transfer_pool", (ng,)), ("energy_recv_pool", (ng,)),
            ("scalars", (4,)),
        ]:
            self.offsets[name] = o
            self.shapes[name] = shape      # C-order shape == reversed Julia shape
            o += int(np.prod(shape))
        self.total = o
        self.n_i64 = ng + IC_COUNT
        self.n_grid = ng

    def view(self, flat: np.ndarray, name: str) -> np.ndarray:
        o = self.offsets[name]
        shp = self.shapes[name]
        return flat[o:o + int(np.prod(shp))].reshape(shp)


# The two kinds of tally sections (the table beside mcs_tally_layout in include/mcs.h): mcs_begin_species resets or sets the
# per-species ones; later species add to the running sums, which mcs_accumulate_tallies moves from one context into another's.
PER_SPECIES_F64 = ("psd", "therm_sf", "therm_pf", "esc_psd_up", "esc_psd_down", "pxx_flux", "pxz_flux", "energy_flux",
                   "energy_recv_pool")
RUNNING_F64 = ("esc_flux", "px_esc_feb", "energy_esc_feb", "esc_energy_eff", "esc_num_eff", "weight_coupled", "spectra_coupled",
               "spectra_sf", "spectra_pf", "energy_transfer_pool", "scalars")


def per_species_i64(L: "Layout") -> slice:
    """num_crossings, [0, n_grid) of the int64 buffer."""
    return slice(0, L.n_grid)


def running_i64(L: "Layout") -> slice:
    """The event counters, [n_grid, n_grid + IC_COUNT)."""
    return slice(L.n_grid, L.n_grid + IC_COUNT)


def _as_dp(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_double_p)


def lib_path() -> str:
    # MCS_HIP_LIB: pick another build of the SAME library (kernel tuning variants)
    name = os.environ.get("MCS_HIP_LIB", "libmcs_hip.so")
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", name)


class MissingNativeLibrary(RuntimeError):
    pass


_LIB = None


def load_library() -> ct.CDLL:
    """Load libmcs_hip.so.  There is NO fallback: the product path is the HIP
    library or nothing (a missing library is an error, never a CPU substitute)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise MissingNativeLibrary(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). No CPU fallback exists for the transport path.")
    lib = ct.CDLL(path)
    vp = ct.c_void_p
    i32, i64, dbl = ct.c_int, ct.c_int64, ct.c_double
    soa_p = ct.POINTER(McsSoa)
    sig = {
        "mcs_abi_version": (i32, []),
        "mcs_last_error": (ct.c_char_p, []),
        "mcs_create": (i32, [ct.POINTER(McsParams), i32, vp, ct.POINTER(vp)]),
        "mcs_destroy": (i32, [vp]),
        "mcs_sync": (i32, [vp]),
        "mcs_bind_tallies": (i32, [vp, vp, i64, vp, i64]),
        "mcs_tallies_f64_devptr": (vp, [vp]),
        "mcs_tallies_i64_devptr": (vp, [vp]),
        "mcs_set_grid": (i32, [vp, i32] + [c_double_p] * 9),
        "mcs_set_cuts": (i32, [vp, i32, c_double_p, i32, c_double_p, i32, c_double_p, c_double_p, c_double_p]),
        "mcs_begin_iteration": (i32, [vp, i32]),
        "mcs_begin_species": (i32, [vp, i32, i32, dbl, dbl, dbl, dbl, dbl]),
        "mcs_set_fluxes": (i32, [vp, c_double_p, c_double_p, c_double_p]),
        "mcs_pop_upload": (i32, [vp, i64, soa_p]),
        "mcs_pop_download": (i32, [vp, i64, soa_p]),
        "mcs_saved_download": (i32, [vp, i64, soa_p, c_uint8_p]),
        "mcs_pop_size": (i64, [vp]),
        "mcs_init_pop": (i32, [vp, i64, i64, i64, c_double_p, c_double_p, dbl, i32, i32, i32]),
        "mcs_init_pop_binned": (i32, [vp, i64, i64, i64, i32, c_double_p, c_double_p, c_int64_p, dbl, i32, i32, i32]),
        "mcs_run_pcut": (i32, [vp, i32, i64, c_int64_p]),
        "mcs_run_pcut_strided": (i32, [vp, i32, i64, i64, c_int64_p]),
        "mcs_run_pcut_indexed": (i32, [vp, i32, vp, c_int64_p]),
        "mcs_saved_gidx": (i32, [vp, i64, vp]),
        "mcs_init_pop_binned_strided": (i32, [vp, i64, i64, i64, i64, i32, c_double_p, c_double_p, c_int64_p, dbl, i32, i32, i32]),
        "mcs_new_pcut": (i32, [vp, i64, c_int64_p]),
        "mcs_saved_export": (i32, [vp, i64, vp, vp, vp]),
        "mcs_split_import": (i32, [vp, i64, i64, vp, vp, i64, i64, i64, i64]),
        "mcs_set_debug_finals": (i32, [vp, i32]),
        "mcs_set_retro_cap": (i32, [vp, i64]),
        "mcs_run_pcut_host": (i32, [vp, i32, i64, i64, soa_p, soa_p, c_uint8_p, c_int64_p]),
        "mcs_read_tallies": (i32, [vp, c_double_p, c_int64_p]),
        "mcs_read_tallies_part": (i32, [vp, i64, i64, c_double_p, c_int64_p]),
        "mcs_write_tallies_part": (i32, [vp, i64, i64, c_double_p]),
        "mcs_num_cus": (i32, [vp]),
        "mcs_write_tallies": (i32, [vp, c_double_p, c_int64_p]),
        "mcs_eval_fn": (i32, [vp, i32, i64, c_double_p, c_double_p, c_double_p]),
        "mcs_eval_scatter": (i32, [vp, i32, i64, c_double_p, c_double_p]),
        "mcs_eval_pcut_split": (i32, [vp, ct.POINTER(McsPcutEval)]),
        "mcs_eval_tally": (i32, [vp, i32, i64, i64, c_double_p, ct.POINTER(ct.c_uint64)]),
        "mcs_eval_move": (i32, [vp, i32, i32, i32, i64, c_double_p, c_double_p, ct.POINTER(ct.c_uint64)]),
        "mcs_eval_pass": (i32, [vp, i32, i32, i64, c_int32_p, c_double_p, ct.POINTER(ct.c_uint64)]),
        "mcs_final_download": (i32, [vp, i64, c_int32_p, c_int32_p, c_int32_p, c_double_p, c_double_p]),
        "mcs_last_kernel_ms": (dbl, [vp]),
        "mcs_set_launch": (i32, [vp, i32, i32]),
        "mcs_set_tail_slicing": (i32, [vp, i32]),
        "mcs_last_launches": (i32, [vp]),
        "mcs_last_kernel": (i32, [vp]),
        "mcs_get_layout": (i32, [ct.POINTER(McsParams), c_int64_p]),
        "mcs_dndp_cr": (i32, [vp, ct.POINTER(McsConsumerIn), c_double_p, c_int64_p]),
        "mcs_thermo_calcs": (i32, [vp, ct.POINTER(McsConsumerIn), c_double_p, c_double_p, c_double_p]),
        "mcs_dndp_esc": (i32, [vp, ct.POINTER(McsConsumerIn), c_double_p, c_double_p, c_double_p, c_int64_p]),
        "mcs_angle_dist": (i32, [vp, ct.POINTER(McsConsumerIn), i32, c_int32_p, c_int32_p, c_double_p, c_double_p, c_double_p]),
        "mcs_tcut_get_layout": (i32, [ct.POINTER(McsParams), i32, ct.POINTER(McsTcutLayout)]),
        "mcs_tcut_spectra": (i32, [vp, ct.POINTER(McsConsumerIn), c_double_p, c_int64_p]),
        "mcs_detector_get_layout": (i32, [ct.POINTER(McsParams), i32, ct.POINTER(McsDetectorLayout)]),
        "mcs_detector_spectra": (i32, [vp, ct.POINTER(McsConsumerIn), i32, i32, dbl, c_double_p, c_int64_p]),
        "mcs_profile_get_layout": (i32, [ct.POINTER(McsParams), ct.POINTER(McsProfileLayout)]),
        "mcs_profile_update": (i32, [vp, ct.POINTER(McsProfileIn), c_double_p, c_double_p, c_int64_p]),
        "mcs_photon_synch": (i32, [vp, c_double_p, c_double_p, dbl, i32, dbl, dbl, c_double_p, c_double_p]),
        "mcs_run_pcuts_fused": (i32, [vp, i32, i32, c_int64_p, c_int64_p, c_int64_p, c_int64_p, c_double_p]),
        "mcs_run_pcuts_pipelined": (i32, [vp, i32, i32, c_int64_p, ct.c_int64, ct.c_int64, c_int64_p, c_int64_p, c_int64_p, c_double_p, c_int64_p]),
        "mcs_dndp_2d": (i32, [vp, ct.POINTER(McsConsumerIn), dbl, dbl, c_double_p]),
        "mcs_photon_ic": (i32, [vp, c_double_p, dbl, i32, i32, c_double_p, c_double_p, i32, dbl, dbl, dbl, c_double_p, c_double_p]),
        "mcs_photon_pion": (i32, [vp, c_double_p, c_double_p, dbl, dbl, c_double_p, dbl, i32, i32, dbl, dbl, c_double_p, c_double_p]),
        "mcs_photon_observe": (i32, [vp, i32, i32, c_double_p, c_double_p, c_double_p, dbl, dbl, dbl, c_double_p, c_double_p, c_double_p, c_double_p,
                               i32, c_int64_p, c_double_p]),
        "mcs_accumulate_tallies": (i32, [vp, vp]),
        "mcs_k1_blocks_per_cu": (i32, [vp]),
        "mcs_option_count": (i32, []),
        "mcs_option_describe": (i32, [i32, ct.POINTER(McsOptionDesc)]),
        "mcs_create_with_options": (i32, [ct.POINTER(McsParams), i32, vp, c_int32_p, c_int64_p, i32, i32, ct.POINTER(vp)]),
        "mcs_set_option": (i32, [vp, i32, i64]),
        "mcs_get_option": (i32, [vp, i32, c_int64_p]),
        "mcs_ens_get_layout": (i32, [ct.POINTER(McsParams), ct.POINTER(McsEnsLayout)]),
        "mcs_ens_create": (i32, [vp, i32, ct.POINTER(vp)]),
        "mcs_ens_destroy": (i32, [vp]),
        "mcs_ens_begin_iteration": (i32, [vp, vp]),
        "mcs_ens_add_species": (i32, [vp, vp, i32]),
        "mcs_ens_add_iteration": (i32, [vp, vp]),
        "mcs_ens_merge": (i32, [vp, vp]),
        "mcs_ens_count": (i32, [vp, i32, c_int64_p]),
        "mcs_ens_read": (i32, [vp, i32, i32, i64, i64, c_double_p]),
        "mcs_ens_load_mean": (i32, [vp, i32, vp]),
        "mcs_ens_summarize": (i32, [vp, i32, i32, ct.POINTER(McsEnsRange), ct.POINTER(McsEnsSummary)]),
        "mcs_ens_summarize_merged": (i32, [i32, ct.POINTER(vp), i32, i32, ct.POINTER(McsEnsRange), ct.POINTER(McsEnsSummary), c_int64_p]),
        "mcs_ens_products_get_layout": (i32, [ct.POINTER(McsParams), ct.POINTER(McsEnsProductsLayout)]),
        "mcs_ens_set_slope_window": (i32, [vp, i32, i32, c_double_p]),
        "mcs_ens_add_products": (i32, [vp, vp, i32]),
        "mcs_ens_photons_get_layout": (i32, [i32, i32, i32, i32, i32, ct.POINTER(McsEnsPhotonsLayout)]),
        "mcs_ens_set_photon_layout": (i32, [vp] + [i32] * 8),
        "mcs_ens_add_photons": (i32, [vp, vp, i32]),
        "mcs_ens_add_photons_deposit": (i32, [vp, vp, i32]),
        "mcs_ens_add_photons_all": (i32, [vp]),
        "mcs_ens_drop_pending_photons": (i32, [vp]),
        "mcs_ens_compare": (i32, [vp, i32, vp, i32, i32, ct.POINTER(McsEnsCmpRange), ct.POINTER(McsEnsDifference)]),
        "mcs_ens_escape_get_layout": (i32, [ct.POINTER(McsParams), ct.POINTER(McsEnsEscapeLayout)]),
        "mcs_ens_add_escape": (i32, [vp, vp, i32]),
        "mcs_ens_angles_get_layout": (i32, [ct.POINTER(McsParams), i32, ct.POINTER(McsEnsAnglesLayout)]),
        "mcs_ens_set_angle_windows": (i32, [vp, i32, c_int32_p, c_int32_p]),
        "mcs_ens_add_angles": (i32, [vp, vp, i32]),
        "mcs_ens_tcuts_get_layout": (i32, [ct.POINTER(McsParams), i32, ct.POINTER(McsTcutLayout)]),
        "mcs_ens_add_tcuts": (i32, [vp, vp, i32]),
        "mcs_ens_profile_get_layout": (i32, [ct.POINTER(McsParams), ct.POINTER(McsProfileLayout)]),
        "mcs_ens_add_profile": (i32, [vp, vp]),
        "mcs_ens_detectors_get_layout": (i32, [ct.POINTER(McsParams), i32, ct.POINTER(McsDetectorLayout)]),
        "mcs_ens_add_detectors": (i32, [vp, vp, i32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    _OPTIONS.clear()
    for key in range(lib.mcs_option_count()):
        d = McsOptionDesc()
        if lib.mcs_option_describe(key, ct.byref(d)) != 0:
            raise RuntimeError("libmcs_hip: " + lib.mcs_last_error().decode())
        _OPTIONS[d.name.decode()] = dict(key=int(d.key), name=d.name.decode(), env=d.env.decode(), min=int(d.min), max=int(d.max),
                                         default=int(d.dflt), when=OPTION_WHEN[d.when], applies=OPTION_APPLIES[d.applies])
    return lib


_OPTIONS: Dict[str, dict] = {}


def tcut_layout(P: McsParams, n_tcuts: int) -> McsTcutLayout:
    """`mcs_tcut_get_layout`: where the parts of a time-cut result of n_tcuts cuts lie (needs no GPU).  ValueError with the library's
    message for an n_tcuts outside 1..99."""
    out = McsTcutLayout()
    lib = load_library()
    if lib.mcs_tcut_get_layout(ct.byref(P), int(n_tcuts), ct.byref(out)) != 0:
        raise ValueError(lib.mcs_last_error().decode())
    return out


def detector_layout(P: McsParams, n_det: int) -> McsDetectorLayout:
    """`mcs_detector_get_layout`: where the parts of a detector result of n_det detectors lie (needs no GPU).  ValueError with the
    library's message for an n_det outside 1..n_grid."""
    out = McsDetectorLayout()
    lib = load_library()
    if lib.mcs_detector_get_layout(ct.byref(P), int(n_det), ct.byref(out)) != 0:
        raise ValueError(lib.mcs_last_error().decode())
    return out


def profile_layout(P: McsParams) -> McsProfileLayout:
    """`mcs_profile_get_layout`: where the rows and scalars of a profile update lie (needs no GPU)."""
    out = McsProfileLayout()
    lib = load_library()
    if lib.mcs_profile_get_layout(ct.byref(P), ct.byref(out)) != 0:
        raise ValueError(lib.mcs_last_error().decode())
    return out


def option_table() -> Dict[str, dict]:
    """The run options of a context, name -> {key, name, env, min, max, default, when, applies}: what the loaded library says
    about itself (mcs_option_describe), read when it is loaded.  include/mcs.h documents every key."""
    load_library()
    return {name: dict(d) for name, d in _OPTIONS.items()}


def option_key(name: str) -> int:
    load_library()
    if name not in _OPTIONS:
        raise KeyError(f"unknown option {name!r}; the library has: {', '.join(_OPTIONS)}")
    return _OPTIONS[name]["key"]


EXPORTED_SYMBOLS = [
    "mcs_abi_version", "mcs_last_error", "mcs_create", "mcs_destroy", "mcs_sync", "mcs_bind_tallies",
    "mcs_tallies_f64_devptr", "mcs_tallies_i64_devptr", "mcs_set_grid", "mcs_set_cuts", "mcs_begin_iteration",
    "mcs_begin_species", "mcs_set_fluxes", "mcs_pop_upload", "mcs_pop_download", "mcs_saved_download",
    "mcs_pop_size", "mcs_init_pop", "mcs_init_pop_binned", "mcs_run_pcut", "mcs_new_pcut", "mcs_run_pcut_host", "mcs_read_tallies", "mcs_read_tallies_part", "mcs_num_cus",
    "mcs_write_tallies", "mcs_eval_fn", "mcs_eval_scatter", "mcs_eval_pcut_split", "mcs_eval_tally", "mcs_eval_move", "mcs_eval_pass", "mcs_final_download", "mcs_last_kernel_ms", "mcs_set_launch",
    "mcs_get_layout", "mcs_dndp_cr", "mcs_thermo_calcs",
    "mcs_run_pcut_strided", "mcs_run_pcut_indexed", "mcs_saved_gidx", "mcs_init_pop_binned_strided", "mcs_saved_export", "mcs_split_import", "mcs_set_debug_finals", "mcs_set_retro_cap",
    "mcs_set_tail_slicing", "mcs_last_launches", "mcs_last_kernel", "mcs_write_tallies_part", "mcs_photon_synch",
    "mcs_dndp_2d", "mcs_photon_ic", "mcs_run_pcuts_fused", "mcs_photon_pion", "mcs_run_pcuts_pipelined",
    "mcs_accumulate_tallies", "mcs_k1_blocks_per_cu",
    "mcs_option_count", "mcs_option_describe", "mcs_create_with_options", "mcs_set_option", "mcs_get_option",
]
# the ensemble statistics (K8)
EXPORTED_SYMBOLS += [
    "mcs_ens_get_layout", "mcs_ens_create", "mcs_ens_destroy", "mcs_ens_begin_iteration", "mcs_ens_add_species",
    "mcs_ens_add_iteration", "mcs_ens_merge", "mcs_ens_count", "mcs_ens_read", "mcs_ens_load_mean", "mcs_ens_summarize",
    "mcs_ens_summarize_merged", "mcs_ens_products_get_layout", "mcs_ens_set_slope_window", "mcs_ens_add_products",
    "mcs_ens_compare",
]
# the observed shell spectra (K9)
EXPORTED_SYMBOLS += ["mcs_photon_observe", "mcs_ens_photons_get_layout", "mcs_ens_set_photon_layout", "mcs_ens_add_photons"]
# the source sample: the photon spectrum summed over species
EXPORTED_SYMBOLS += ["mcs_ens_add_photons_deposit", "mcs_ens_add_photons_all", "mcs_ens_drop_pending_photons"]
# the spectra of the escaping particles (K10) and their sample
EXPORTED_SYMBOLS += ["mcs_dndp_esc", "mcs_ens_escape_get_layout", "mcs_ens_add_escape"]
# the pitch-angle distributions (K11) and their sample
EXPORTED_SYMBOLS += ["mcs_angle_dist", "mcs_ens_angles_get_layout", "mcs_ens_set_angle_windows", "mcs_ens_add_angles"]
# the time-cut spectra (K12) and their sample
EXPORTED_SYMBOLS += ["mcs_tcut_spectra", "mcs_tcut_get_layout", "mcs_ens_tcuts_get_layout", "mcs_ens_add_tcuts"]
# the shock-profile update (K13) and its sample
EXPORTED_SYMBOLS += ["mcs_profile_update", "mcs_profile_get_layout", "mcs_ens_profile_get_layout", "mcs_ens_add_profile"]
# the detector spectra (K14) and their sample
EXPORTED_SYMBOLS += ["mcs_detector_spectra", "mcs_detector_get_layout", "mcs_ens_detectors_get_layout", "mcs_ens_add_detectors"]
PHOTON_PROCESS = {"synch": 0, "ic": 1, "pion": 2}      # MCS_PHOTON_SYNCH, _IC, _PION
