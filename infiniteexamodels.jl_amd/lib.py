"""ctypes binding of ``libiem_hip.so`` (the C-ABI of ``include/iem.h``).

The library is the product path: if it is missing this module raises — there is no
Python/CPU fallback for evaluation.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libiem_hip.so")
KERNEL_DIR = os.path.join(_HERE, "kernels")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

_lib = None
DEFAULT_STORE_MODE = 2


class IemError(RuntimeError):
    pass


IEM_E_ARG = -4      # (include/iem.h)


class Meta(C.Structure):
    _fields_ = [("nvar", C.c_int64), ("ncon", C.c_int64), ("npar", C.c_int64), ("nnzj", C.c_int64),
                ("nnzh", C.c_int64), ("n_templates", C.c_int64), ("minimize", C.c_int32),
                ("n_kernels", C.c_int32)]


class TemplateInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("kind", "n_items", "o0", "o1", "o2", "o1step", "o2step")]


class Option(C.Structure):
    _fields_ = [("name", C.c_char_p), ("value", C.c_int64)]


class ShardT(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("group", "rank", "world", "mailbox_kind")] + \
               [(n, C.c_int64) for n in ("n_global", "own_lo", "own_n", "halo", "halo_reach", "halo_doubles", "nvar_global",
                                         "ncon_global", "nnzj_global", "nnzh_global", "nvar", "ncon", "nnzj", "nnzh",
                                         "n_templates", "n_shared")]

    def asdict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class ShardTemplate(C.Structure):
    _fields_ = [("global_index", C.c_int64), ("kind", C.c_int64), ("n_items", C.c_int64), ("klo", C.c_int64 * 3),
                ("dims", C.c_int64 * 3), ("global_dims", C.c_int64 * 3)] + \
               [(n, C.c_int64) for n in ("o0", "o1", "o2", "global_o0", "global_o1", "global_o2", "o1step", "o2step", "items_offset")]

    def asdict(self, items=None):
        """``items``: the concatenated explicit item lists; adds ``ordinals`` = global item ordinal of every local item."""
        import numpy as np
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d = {k: (tuple(int(x) for x in v) if hasattr(v, "__len__") else int(v)) for k, v in d.items()}
        if d["items_offset"] >= 0:
            d["ordinals"] = np.asarray(items[d["items_offset"]:d["items_offset"] + d["n_items"]], dtype=np.int64)
        else:
            k0, k1, k2 = (np.arange(n) for n in d["dims"])
            g0, g1, _ = d["global_dims"]
            d["ordinals"] = ((d["klo"][0] + k0)[None, None, :] + g0 * ((d["klo"][1] + k1)[None, :, None]
                             + g1 * (d["klo"][2] + k2)[:, None, None])).reshape(-1)
        return d


COMM_HANDLE_BYTES = 128


class KktInfo(C.Structure):
    _fields_ = [("S", C.c_int64), ("n", C.c_int64), ("n_border", C.c_int64), ("block_doubles", C.c_int64),
                ("nb", C.c_int32), ("ne", C.c_int32), ("nc", C.c_int32), ("reach", C.c_int32), ("group", C.c_int32), ("phase", C.c_int32),
                ("lanes", C.c_int64), ("hub_ld", C.c_int64), ("hubs", C.c_int32), ("hub_rows", C.c_int32), ("hubs_per_block", C.c_int32), ("reserved_", C.c_int32)]


class BarrierInfo(C.Structure):
    """``iem_barrier_info_t``: ``struct_size`` is set by the caller; the library writes at most that many bytes."""
    _fields_ = [("struct_size", C.c_uint64)] + [(n, C.c_int64) for n in ("nvar", "ncon", "n_eq", "n_ineq", "n_xl", "n_xu", "n_sl", "n_su", "nz", "workgroups")]


class SearchOpts(C.Structure):
    """``iem_search_opts_t``: ``struct_size`` is set by the caller; ``SearchOpts.defaults()`` has Ipopt's values."""
    _fields_ = ([("struct_size", C.c_uint64)] + [(n, C.c_double) for n in ("gamma_theta", "gamma_phi", "eta_phi", "delta", "s_theta", "s_phi", "alpha_floor")] +
                [(n, C.c_int64) for n in ("max_trials", "filter_capacity")])
    DEFAULTS = dict(gamma_theta=1e-5, gamma_phi=1e-8, eta_phi=1e-8, delta=1.0, s_theta=1.1, s_phi=2.3, alpha_floor=1e-16, max_trials=30, filter_capacity=64)

    @classmethod
    def defaults(cls, **over):
        unknown = set(over) - set(cls.DEFAULTS)
        if unknown:
            raise TypeError(f"unknown search option(s): {sorted(unknown)}")
        o = cls(**{**cls.DEFAULTS, **over})
        o.struct_size = C.sizeof(cls)
        return o


class SearchState(C.Structure):
    """``iem_search_state_t``: ``struct_size`` (set by the caller), then words 0-12 of the control block."""
    _fields_ = ([("struct_size", C.c_uint64)] +
                [(n, C.c_double) for n in ("alpha", "alpha_max", "phi0", "theta0", "slope", "theta_min", "theta_max", "phi_trial", "theta_trial")] +
                [(n, C.c_int64) for n in ("status", "trials", "filter_count", "flags")])


SEARCH_STATUS = ("searching", "accepted_f", "accepted_h", "failed", "unusable")


class SocOpts(C.Structure):
    """``iem_soc_opts_t``: ``struct_size`` is set by the caller; ``SocOpts.defaults()`` has Ipopt's values."""
    _fields_ = [("struct_size", C.c_uint64), ("max_soc", C.c_int64), ("kappa_soc", C.c_double)]
    DEFAULTS = dict(max_soc=4, kappa_soc=0.99)

    @classmethod
    def defaults(cls, **over):
        unknown = set(over) - set(cls.DEFAULTS)
        if unknown:
            raise TypeError(f"unknown second-order correction option(s): {sorted(unknown)}")
        o = cls(**{**cls.DEFAULTS, **over})
        o.struct_size = C.sizeof(cls)
        return o


class SocState(C.Structure):
    """``iem_soc_state_t``: ``struct_size`` (set by the caller), the status word, then words 13-15 of the control block."""
    _fields_ = [("struct_size", C.c_uint64), ("status", C.c_int64), ("state", C.c_int64), ("rounds", C.c_int64), ("alpha_prev", C.c_double)]


SOC_STATE = ("none", "active", "accepted", "closed")


class RestoOpts(C.Structure):
    """``iem_resto_opts_t``: ``struct_size`` is set by the caller; ``RestoOpts.defaults()`` has Ipopt's values."""
    _fields_ = [("struct_size", C.c_uint64), ("rho", C.c_double), ("kappa_resto", C.c_double), ("bound_mult_reset_threshold", C.c_double)]
    DEFAULTS = dict(rho=1000.0, kappa_resto=0.9, bound_mult_reset_threshold=1000.0)

    @classmethod
    def defaults(cls, **over):
        unknown = set(over) - set(cls.DEFAULTS)
        if unknown:
            raise TypeError(f"unknown restoration option(s): {sorted(unknown)}")
        o = cls(**{**cls.DEFAULTS, **over})
        o.struct_size = C.sizeof(cls)
        return o


class RestoState(C.Structure):
    """``iem_resto_state_t``: ``struct_size`` (set by the caller), then words 0-3 of the object's block."""
    _fields_ = [("struct_size", C.c_uint64), ("state", C.c_int64), ("theta_start", C.c_double), ("theta", C.c_double), ("phi", C.c_double)]


RESTO_STATE = ("none", "active", "return")


class MuOpts(C.Structure):
    """``iem_mu_opts_t``: ``struct_size`` is set by the caller; ``MuOpts.defaults()`` has Ipopt's values (``mu_floor = 0``: the library
    takes ``max(1e-11, tol/10)``)."""
    _fields_ = [("struct_size", C.c_uint64)] + [(n, C.c_double) for n in ("mu_init", "kappa_eps", "kappa_mu", "tau_min", "tol", "mu_floor", "s_max")]
    DEFAULTS = dict(mu_init=0.1, kappa_eps=10.0, kappa_mu=0.2, tau_min=0.99, tol=1e-8, mu_floor=0.0, s_max=100.0)

    @classmethod
    def defaults(cls, **over):
        unknown = set(over) - set(cls.DEFAULTS)
        if unknown:
            raise TypeError(f"unknown barrier parameter option(s): {sorted(unknown)}")
        o = cls(**{**cls.DEFAULTS, **over})
        o.struct_size = C.sizeof(cls)
        return o


class MuState(C.Structure):
    """``iem_mu_state_t``: ``struct_size`` (set by the caller), then words 0-11 of the object's block."""
    _fields_ = ([("struct_size", C.c_uint64)] + [(n, C.c_double) for n in ("mu", "tau", "zeta", "e0", "e_mu", "e_d", "e_p", "e_c0")] +
                [(n, C.c_int64) for n in ("status", "flags", "decreases", "updates")])


MU_STATUS = ("iterating", "converged", "unusable")


class AmuOpts(C.Structure):
    """``iem_amu_opts_t``: ``struct_size`` is set by the caller; ``AmuOpts.defaults()`` has the library's values (``oracle``: 0 probing,
    1 LOQO — or the names of ``AMU_ORACLE``)."""
    _fields_ = ([("struct_size", C.c_uint64), ("oracle", C.c_int64)] +
                [(n, C.c_double) for n in ("sigma_max", "mu_min", "mu_max_fact", "init_factor", "red_fact")] + [("refs_max", C.c_int64)])
    DEFAULTS = dict(oracle=0, sigma_max=100.0, mu_min=1e-11, mu_max_fact=1e3, init_factor=0.8, red_fact=0.9999, refs_max=4)

    @classmethod
    def defaults(cls, **over):
        unknown = set(over) - set(cls.DEFAULTS)
        if unknown:
            raise TypeError(f"unknown adaptive barrier parameter option(s): {sorted(unknown)}")
        if isinstance(over.get("oracle"), str):
            if over["oracle"] not in AMU_ORACLE:
                raise ValueError(f"oracle: one of {AMU_ORACLE} expected, got {over['oracle']!r}")
            over["oracle"] = AMU_ORACLE.index(over["oracle"])
        o = cls(**{**cls.DEFAULTS, **over})
        o.struct_size = C.sizeof(cls)
        return o


class AmuState(C.Structure):
    """``iem_amu_state_t``: ``struct_size`` (set by the caller), then words 0-13 of the object's own block."""
    _fields_ = [("struct_size", C.c_uint64), ("mode", C.c_int64), ("mu_max", C.c_double), ("refs_count", C.c_int64), ("refs", C.c_double * 4),
                ("mu_oracle", C.c_double), ("sigma", C.c_double), ("avg", C.c_double), ("m_aff", C.c_double),
                ("to_fixed", C.c_int64), ("to_free", C.c_int64), ("oracle", C.c_int64)]


AMU_MODE = ("free", "fixed")
AMU_ORACLE = ("probing", "loqo")


class QfOpts(C.Structure):
    """``iem_qf_opts_t``: ``struct_size`` is set by the caller; ``QfOpts.defaults()`` has the library's values (``sigma_max = 0``: the
    ``iem_amu`` object's)."""
    _fields_ = ([("struct_size", C.c_uint64)] + [(n, C.c_double) for n in ("mu_ref", "sigma_min", "sigma_max", "section_sigma_tol")] +
                [("max_section_steps", C.c_int64)])
    DEFAULTS = dict(mu_ref=1.0, sigma_min=1e-6, sigma_max=0.0, section_sigma_tol=1e-2, max_section_steps=8)

    @classmethod
    def defaults(cls, **over):
        unknown = set(over) - set(cls.DEFAULTS)
        if unknown:
            raise TypeError(f"unknown quality-function option(s): {sorted(unknown)}")
        o = cls(**{**cls.DEFAULTS, **over})
        o.struct_size = C.sizeof(cls)
        return o


class QfState(C.Structure):
    """``iem_qf_state_t``: ``struct_size`` (set by the caller), then words 0-26 of the object's own block."""
    _fields_ = ([("struct_size", C.c_uint64)] + [(n, C.c_int64) for n in ("status", "phase", "steps", "evaluations")] +
                [("sigma_trial", C.c_double), ("alpha_slots", C.c_double * 2)] +
                [(n, C.c_double) for n in ("d2", "p2", "avg", "lo", "hi", "a", "b", "c", "d", "qc", "qd", "sigma", "q", "q_first",
                                           "q_last", "c2_last", "nan_last", "alpha_p_last", "alpha_d_last", "sigma_first")])


QF_STATUS = ("idle", "section", "done", "unusable")


class MpcOpts(C.Structure):
    """``iem_mpc_opts_t``: ``struct_size`` is set by the caller; ``MpcOpts.defaults()`` has the library's value (Ipopt's
    ``corrector_compl_avrg_red_fact``)."""
    _fields_ = [("struct_size", C.c_uint64), ("red_fact", C.c_double)]
    DEFAULTS = dict(red_fact=1.0)

    @classmethod
    def defaults(cls, **over):
        unknown = set(over) - set(cls.DEFAULTS)
        if unknown:
            raise TypeError(f"unknown corrector option(s): {sorted(unknown)}")
        o = cls(**{**cls.DEFAULTS, **over})
        o.struct_size = C.sizeof(cls)
        return o


class MpcState(C.Structure):
    """``iem_mpc_state_t``: ``struct_size`` (set by the caller), then words 0-6 of the object's own block."""
    _fields_ = ([("struct_size", C.c_uint64)] + [(n, C.c_int64) for n in ("taken", "n_taken", "n_refused")] +
                [("predicted", C.c_double), ("avg", C.c_double), ("alpha_c", C.c_double * 2)])


class InitOpts(C.Structure):
    """``iem_init_opts_t``: ``struct_size`` is set by the caller; ``InitOpts.defaults()`` has the library's values (Ipopt's
    ``constr_mult_init_max``, its initialiser's ``y = 0`` on rejection, ``warm_start_bound_push``, ``warm_start_bound_frac``,
    ``warm_start_mult_bound_push``, ``warm_start_mult_init_max``; ``mu_cap = 0``: the ``mu_init`` of the bound parameter)."""
    _fields_ = ([("struct_size", C.c_uint64), ("y_max", C.c_double), ("on_reject", C.c_int64)] +
                [(n, C.c_double) for n in ("warm_push", "warm_frac", "warm_z_push", "warm_z_max", "warm_y_max", "mu_factor", "mu_cap")])
    DEFAULTS = dict(y_max=1e3, on_reject=0, warm_push=1e-3, warm_frac=1e-3, warm_z_push=1e-3, warm_z_max=1e6, warm_y_max=1e6, mu_factor=1.0, mu_cap=0.0)

    @classmethod
    def defaults(cls, **over):
        unknown = set(over) - set(cls.DEFAULTS)
        if unknown:
            raise TypeError(f"unknown starting-point option(s): {sorted(unknown)}")
        o = cls(**{**cls.DEFAULTS, **over})
        o.struct_size = C.sizeof(cls)
        return o


class InitState(C.Structure):
    """``iem_init_state_t``: ``struct_size`` (set by the caller), then words 0-5 of the object's own block."""
    _fields_ = ([("struct_size", C.c_uint64), ("ynorm", C.c_double)] + [(n, C.c_int64) for n in ("accepted", "n_accepted", "n_rejected")] +
                [("mu0", C.c_double), ("how", C.c_int64)])


INIT_HOW = ("average", "fallback", "clamped_below", "clamped_above")


class ConvOpts(C.Structure):
    """``iem_conv_opts_t``: ``struct_size`` is set by the caller; ``ConvOpts.defaults()`` has the library's values (Ipopt's
    ``dual_inf_tol``, ``constr_viol_tol``, ``compl_inf_tol``, ``acceptable_*``, ``max_iter``, ``diverging_iterates_tol``,
    ``tiny_step_tol`` = ten machine epsilons, ``tiny_step_y_tol``).  ``+inf`` switches a tolerance off."""
    _fields_ = ([("struct_size", C.c_uint64)] + [(n, C.c_double) for n in ("dual_inf_tol", "constr_viol_tol", "compl_inf_tol", "acceptable_tol")] +
                [("acceptable_iter", C.c_int64)] +
                [(n, C.c_double) for n in ("acceptable_dual_inf_tol", "acceptable_constr_viol_tol", "acceptable_compl_inf_tol", "acceptable_obj_change_tol")] +
                [("max_iter", C.c_int64)] + [(n, C.c_double) for n in ("diverging_iterates_tol", "tiny_step_tol", "tiny_step_y_tol")])
    DEFAULTS = dict(dual_inf_tol=1.0, constr_viol_tol=1e-4, compl_inf_tol=1e-4, acceptable_tol=1e-6, acceptable_iter=15, acceptable_dual_inf_tol=1e10,
                    acceptable_constr_viol_tol=1e-2, acceptable_compl_inf_tol=1e-2, acceptable_obj_change_tol=1e20, max_iter=3000, diverging_iterates_tol=1e20,
                    tiny_step_tol=10.0 * 2.0 ** -52, tiny_step_y_tol=1e-2)

    @classmethod
    def defaults(cls, **over):
        unknown = set(over) - set(cls.DEFAULTS)
        if unknown:
            raise TypeError(f"unknown stopping-test option(s): {sorted(unknown)}")
        o = cls(**{**cls.DEFAULTS, **over})
        o.struct_size = C.sizeof(cls)
        return o


class ConvState(C.Structure):
    """``iem_conv_state_t``: ``struct_size`` (set by the caller), then words 0-18 of the object's own block."""
    _fields_ = ([("struct_size", C.c_uint64)] + [(n, C.c_int64) for n in ("status", "checks", "acceptable_count", "keep", "kept", "kept_at", "flags", "tiny_count")] +
                [(n, C.c_double) for n in ("e0", "dual_inf", "constr_viol", "compl_inf", "f", "f_prev", "xmax", "kept_e0", "kept_f", "rel", "dymax")])


CONV_STATUS = ("iterating", "converged", "acceptable", "maxiter", "diverging", "invalid", "tiny_step")


class RmuOpts(C.Structure):
    """``iem_rmu_opts_t``: ``struct_size`` is set by the caller; ``RmuOpts.defaults()`` has the library's values (Ipopt's
    ``barrier_tol_factor``, ``mu_linear_decrease_factor``, ``tau_min``, ``tol``, the floor of mu, ``s_max``, ``alpha_min_frac``)."""
    _fields_ = [("struct_size", C.c_uint64)] + [(n, C.c_double) for n in ("kappa_eps", "kappa_mu", "tau_min", "tol", "mu_floor", "s_max", "gamma_alpha")]
    DEFAULTS = dict(kappa_eps=10.0, kappa_mu=0.2, tau_min=0.99, tol=1e-8, mu_floor=1e-11, s_max=100.0, gamma_alpha=0.05)

    @classmethod
    def defaults(cls, **over):
        unknown = set(over) - set(cls.DEFAULTS)
        if unknown:
            raise TypeError(f"unknown restoration parameter option(s): {sorted(unknown)}")
        o = cls(**{**cls.DEFAULTS, **over})
        o.struct_size = C.sizeof(cls)
        return o


class RmuState(C.Structure):
    """``iem_rmu_state_t``: ``struct_size`` (set by the caller), then words 0-10 of the object's own block, words 0-11 of the
    restoration ``iem_mu`` block and words 0-3 of the ``iem_resto`` block — one copy."""
    _fields_ = ([("struct_size", C.c_uint64)] + [(n, C.c_int64) for n in ("status", "flags", "decreases_last", "decreases")] +
                [(n, C.c_double) for n in ("e0", "e_mu", "mu_enter", "inf_enter", "alpha_min")] + [(n, C.c_int64) for n in ("triggers_orig", "triggers_inner")] +
                [(n, C.c_double) for n in ("mu", "tau", "zeta", "mu_e0", "mu_e_mu", "mu_e_d", "mu_e_p", "mu_e_c0")] +
                [(n, C.c_int64) for n in ("mu_status", "mu_flags", "mu_decreases", "mu_updates")] +
                [("resto_state", C.c_int64)] + [(n, C.c_double) for n in ("theta_start", "theta", "phi")])


RMU_STATUS = ("iterating", "stationary", "unusable")
RMU_K = 6


class KernelInfo(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("kind", C.c_int32), ("jit", C.c_int32), ("grid", C.c_int64 * 3),
                ("lds_bytes", C.c_int64), ("alg_bytes_read", C.c_int64), ("alg_bytes_written", C.c_int64)]


# every symbol include/iem.h declares (tests check the export list against the header)
SYMBOLS = ["iem_create", "iem_create_opts", "iem_create_sharded", "iem_shard_info", "iem_shard_halo", "iem_shard_var_map", "iem_shard_template_info",
           "iem_shard_template_items", "iem_shard_blob", "iem_comm_export", "iem_comm_connect", "iem_halo_exchange", "iem_halo_exchange_async", "iem_halo_wait", "iem_halo_reads", "iem_halo_fold", "iem_allreduce_obj_grad", "iem_comm_status",
           "iem_destroy", "iem_meta", "iem_template_info", "iem_kernel_info", "iem_get_host", "iem_set_stream",
           "iem_synchronize", "iem_set_parameter", "iem_obj", "iem_obj_device", "iem_obj_begin", "iem_obj_end", "iem_grad", "iem_cons",
           "iem_jac_coord", "iem_hess_coord", "iem_jac_hess_coord", "iem_eval_trial", "iem_eval_accepted", "iem_eval_all", "iem_lagrad_prepare", "iem_lagrad", "iem_eval_residual", "iem_scaled_prepare", "iem_jac_rowmax", "iem_cons_scaled", "iem_jac_coord_scaled", "iem_scaled_phase_prepare", "iem_grad_scaled", "iem_hess_coord_scaled", "iem_eval_trial_scaled", "iem_eval_accepted_scaled", "iem_kktprod_prepare", "iem_kktprod", "iem_jprod", "iem_jtprod", "iem_hprod", "iem_param_prepare", "iem_jpprod", "iem_jptprod", "iem_hpprod", "iem_hptprod", "iem_hppprod_prepare", "iem_hppprod", "iem_param_coord_prepare", "iem_kernel_count", "iem_param_coord_nnz", "iem_jacp_structure", "iem_hessxp_structure", "iem_hesspp_structure", "iem_jacp_coord", "iem_hessp_coord", "iem_jac_structure", "iem_hess_structure",
           "iem_jac_structure_device", "iem_hess_structure_device", "iem_csr_values", "iem_csr_values32", "iem_csr_spmv", "iem_kkt_chain_factor", "iem_kkt_chain_level", "iem_kkt_hub_level", "iem_kkt_chain_solve", "iem_kkt_chain_solve_lanes", "iem_kkt_chain_solve_many", "iem_kkt_source", "iem_kkt_create", "iem_kkt_destroy", "iem_kkt_info", "iem_kkt_layout", "iem_kkt_analyse_blob", "iem_kkt_assemble", "iem_kkt_factor", "iem_kkt_solve", "iem_kkt_solve_many", "iem_kkt_residual", "iem_kkt_solve_refined", "iem_kkt_assemble_diag", "iem_kkt_residual_diag", "iem_kkt_solve_refined_diag", "iem_kkt_diag_source", "iem_kkt_border_factor", "iem_kkt_border_solve", "iem_kkt_border_source", "iem_kkt_set_border", "iem_kkt_factor_async", "iem_barrier_create", "iem_barrier_analyse", "iem_barrier_destroy", "iem_barrier_info", "iem_barrier_start", "iem_barrier_terms", "iem_barrier_step", "iem_barrier_update", "iem_barrier_error", "iem_barrier_merit", "iem_barrier_source", "iem_search_create", "iem_search_destroy", "iem_search_reset", "iem_search_begin", "iem_search_trial", "iem_search_accept", "iem_search_device", "iem_search_state", "iem_search_source", "iem_soc_create", "iem_soc_destroy", "iem_soc_open", "iem_soc_rhs", "iem_soc_trial", "iem_soc_accept", "iem_soc_select", "iem_soc_device", "iem_soc_state", "iem_soc_source", "iem_resto_create", "iem_resto_destroy", "iem_resto_search", "iem_resto_enter", "iem_resto_terms", "iem_resto_step", "iem_resto_merit", "iem_resto_begin", "iem_resto_trial", "iem_resto_update", "iem_resto_error", "iem_resto_check", "iem_resto_leave", "iem_resto_device", "iem_resto_state", "iem_resto_source", "iem_mu_create", "iem_mu_destroy", "iem_mu_reset", "iem_mu_error", "iem_mu_update", "iem_mu_device", "iem_mu_state", "iem_barrier_bind_mu", "iem_search_bind_mu", "iem_soc_bind_mu", "iem_mu_source", "iem_barrier_mu_source", "iem_amu_create", "iem_amu_destroy", "iem_amu_reset", "iem_amu_probe", "iem_amu_update", "iem_amu_device", "iem_amu_state", "iem_amu_source", "iem_qf_create", "iem_qf_destroy", "iem_qf_reset", "iem_qf_begin", "iem_qf_alpha", "iem_qf_value", "iem_qf_update", "iem_qf_device", "iem_qf_state", "iem_qf_source", "iem_mpc_create", "iem_mpc_destroy", "iem_mpc_reset", "iem_mpc_bind_mu", "iem_mpc_terms", "iem_mpc_step", "iem_mpc_select", "iem_mpc_device", "iem_mpc_state", "iem_mpc_source", "iem_init_create", "iem_init_destroy", "iem_init_reset", "iem_init_ls_terms", "iem_init_ls_apply", "iem_init_warm", "iem_init_mu", "iem_init_device", "iem_init_state", "iem_init_source", "iem_conv_create", "iem_conv_destroy", "iem_conv_reset", "iem_conv_check", "iem_conv_keep", "iem_conv_restore", "iem_conv_step", "iem_conv_kept", "iem_conv_device", "iem_conv_state", "iem_conv_source", "iem_rmu_create", "iem_rmu_destroy", "iem_rmu_mu", "iem_rmu_enter", "iem_rmu_error", "iem_rmu_update", "iem_rmu_trigger", "iem_rmu_device", "iem_rmu_state", "iem_resto_bind_mu", "iem_rmu_source", "iem_resto_mu_source", "iem_emit_source", "iem_fixed_source", "iem_emit_launch_plan", "iem_blob_hess_structure", "iem_blob_param_coord_structure", "iem_blob_array", "iem_free",
           "iem_set_option", "iem_time_kernels", "iem_tuner_choice", "iem_tune", "iem_last_error", "iem_version"]


def build_library(force: bool = False) -> str:
    """Compile ``libiem_hip.so`` in-tree (host C++; links libamdhip64 + libhiprtc)."""
    src_dir = os.path.join(_HERE, "csrc")
    newest = max(os.path.getmtime(os.path.join(src_dir, f)) for f in os.listdir(src_dir)
                 if f.endswith((".cpp", ".hpp", ".h", "Makefile")))
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < newest:
        subprocess.check_call(["make", "-C", src_dir, "-s"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IemError(f"{LIB_PATH} is missing — run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback for the evaluation path)")
    # One HIP runtime per process: torch (this binding's device-memory provider) ships its own
    # libamdhip64; if libiem_hip.so pulled in the system one FIRST, the two runtimes coexist and
    # the second to initialise sees no device.  Loading torch first makes libiem_hip bind to the
    # runtime torch already loaded (same SONAME).  C / Julia hosts link one runtime and are not
    # affected.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i64, dbl, i32 = C.c_void_p, C.c_int64, C.c_double, C.c_int
    L.iem_last_error.restype = C.c_char_p
    L.iem_version.restype = C.c_char_p
    L.iem_create.argtypes = [C.c_char_p, C.c_size_t, i32, C.POINTER(vp)]
    L.iem_create_opts.argtypes = [C.c_char_p, C.c_size_t, i32, C.POINTER(Option), i32, C.POINTER(vp)]
    L.iem_create_sharded.argtypes = [C.c_char_p, C.c_size_t, i32, i32, i32, i32, C.POINTER(Option), i32, C.POINTER(vp)]
    L.iem_shard_info.argtypes = [vp, C.POINTER(ShardT)]
    L.iem_shard_var_map.argtypes = [vp, vp, vp]
    L.iem_shard_halo.argtypes = [vp, C.POINTER(C.c_int64 * 6)]
    L.iem_shard_template_info.argtypes = [vp, i64, C.POINTER(ShardTemplate)]
    L.iem_shard_blob.argtypes = [C.c_char_p, C.c_size_t, i32, i32, i32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(ShardT),
                                 C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.iem_shard_template_items.argtypes = [vp, vp, C.POINTER(C.c_int64)]
    L.iem_comm_export.argtypes = [vp, vp]
    L.iem_comm_connect.argtypes = [vp, vp]
    L.iem_halo_exchange.argtypes = [vp, vp]
    L.iem_halo_exchange_async.argtypes = [vp, vp]
    L.iem_halo_wait.argtypes = [vp]
    L.iem_halo_reads.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.iem_halo_fold.argtypes = [vp, vp]
    L.iem_allreduce_obj_grad.argtypes = [vp, vp, vp]
    L.iem_comm_status.argtypes = [vp, C.POINTER(C.c_int64)]
    L.iem_destroy.argtypes = [vp]
    L.iem_meta.argtypes = [vp, C.POINTER(Meta)]
    L.iem_template_info.argtypes = [vp, i64, C.POINTER(TemplateInfo)]
    L.iem_kernel_info.argtypes = [vp, i32, C.POINTER(KernelInfo)]
    L.iem_get_host.argtypes = [vp, i32, vp]
    L.iem_set_stream.argtypes = [vp, vp]
    L.iem_synchronize.argtypes = [vp]
    L.iem_set_parameter.argtypes = [vp, i64, i64, vp]
    L.iem_obj.argtypes = [vp, vp, C.POINTER(dbl)]
    L.iem_obj_device.argtypes = [vp, vp, vp]
    L.iem_obj_begin.argtypes = [vp, vp]
    L.iem_obj_end.argtypes = [vp, C.POINTER(dbl)]
    L.iem_jac_hess_coord.argtypes = [vp, vp, vp, dbl, vp, vp]
    L.iem_eval_trial.argtypes = [vp, vp, vp, C.POINTER(dbl)]
    L.iem_eval_accepted.argtypes = [vp, vp, vp, dbl, vp, vp, vp]
    L.iem_eval_all.argtypes = [vp, vp, vp, dbl, vp, vp, vp, vp, C.POINTER(dbl)]
    L.iem_lagrad_prepare.argtypes = [vp, C.POINTER(C.c_int32)]
    L.iem_lagrad.argtypes = [vp, vp, vp, dbl, vp]
    L.iem_eval_residual.argtypes = [vp, vp, vp, dbl, vp, vp, vp]
    L.iem_scaled_prepare.argtypes = [vp, C.POINTER(C.c_int32)]
    L.iem_jac_rowmax.argtypes = [vp, vp, vp]
    L.iem_cons_scaled.argtypes = [vp, vp, vp, vp]
    L.iem_jac_coord_scaled.argtypes = [vp, vp, vp, vp]
    L.iem_scaled_phase_prepare.argtypes = [vp, C.POINTER(C.c_int32)]
    L.iem_grad_scaled.argtypes = [vp, vp, dbl, vp]
    L.iem_hess_coord_scaled.argtypes = [vp, vp, vp, vp, dbl, vp]
    L.iem_eval_trial_scaled.argtypes = [vp, vp, vp, dbl, vp, C.POINTER(dbl)]
    L.iem_eval_accepted_scaled.argtypes = [vp, vp, vp, vp, dbl, dbl, vp, vp, vp]
    L.iem_kktprod_prepare.argtypes = [vp, C.POINTER(C.c_int32)]
    L.iem_kktprod.argtypes = [vp, vp, vp, dbl, vp, vp, vp, vp]
    L.iem_grad.argtypes = [vp, vp, vp]
    L.iem_cons.argtypes = [vp, vp, vp]
    L.iem_jac_coord.argtypes = [vp, vp, vp]
    L.iem_hess_coord.argtypes = [vp, vp, vp, dbl, vp]
    L.iem_jprod.argtypes = [vp, vp, vp, vp]
    L.iem_jtprod.argtypes = [vp, vp, vp, vp]
    L.iem_hprod.argtypes = [vp, vp, vp, vp, dbl, vp]
    L.iem_param_prepare.argtypes = [vp, C.POINTER(C.c_int32)]
    L.iem_jpprod.argtypes = [vp, vp, vp, vp]
    L.iem_jptprod.argtypes = [vp, vp, vp, dbl, vp]
    L.iem_hpprod.argtypes = [vp, vp, vp, dbl, vp, vp]
    L.iem_hptprod.argtypes = [vp, vp, vp, dbl, vp, vp]
    L.iem_hppprod_prepare.argtypes = [vp, C.POINTER(C.c_int32)]
    L.iem_hppprod.argtypes = [vp, vp, vp, dbl, vp, vp]
    L.iem_param_coord_prepare.argtypes = [vp, C.POINTER(C.c_int32)]
    L.iem_param_coord_nnz.argtypes = [vp, C.POINTER(C.c_int64 * 3)]
    L.iem_kernel_count.argtypes = [vp, C.POINTER(C.c_int32)]
    L.iem_jacp_coord.argtypes = [vp, vp, vp]
    L.iem_hessp_coord.argtypes = [vp, vp, vp, dbl, vp, vp]
    for f in ("iem_jac_structure", "iem_hess_structure", "iem_jac_structure_device", "iem_hess_structure_device", "iem_jacp_structure", "iem_hessxp_structure",
              "iem_hesspp_structure"):
        getattr(L, f).argtypes = [vp, vp, vp, i32]
    L.iem_csr_values.argtypes = [vp, i64, vp, vp, vp, vp]
    L.iem_csr_values32.argtypes = [vp, i64, vp, vp, vp, vp]
    L.iem_csr_spmv.argtypes = [vp, i64, vp, vp, vp, vp, vp, i64, vp]
    L.iem_kkt_chain_factor.argtypes = [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, dbl]
    L.iem_kkt_chain_level.argtypes = [vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, dbl, i64, i32]
    L.iem_kkt_hub_level.argtypes = [vp, i64, i64, i32, i32, vp, vp, vp, i32, vp, i32, vp, i32, i32, i64, vp, vp, vp, i32]
    L.iem_kkt_chain_solve.argtypes = [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32]
    L.iem_kkt_chain_solve_lanes.argtypes = [vp, i64, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32]
    L.iem_kkt_chain_solve_many.argtypes = [vp, i64, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    L.iem_kkt_source.argtypes = [i32, i32, i32, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_kkt_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.iem_kkt_destroy.argtypes = [vp]
    L.iem_kkt_info.argtypes = [vp, C.POINTER(KktInfo)]
    L.iem_kkt_layout.argtypes = [vp, vp, vp, vp, vp]
    L.iem_kkt_analyse_blob.argtypes = [vp, C.c_size_t, i32, C.POINTER(KktInfo)] + [C.POINTER(vp)] * 7 + [C.POINTER(i64), C.POINTER(i64)]
    L.iem_kkt_assemble.argtypes = [vp, vp, vp, vp, dbl, dbl]
    L.iem_kkt_factor.argtypes = [vp, vp]
    L.iem_kkt_solve.argtypes = [vp, vp, vp]
    L.iem_kkt_solve_many.argtypes = [vp, i32, vp, i64, vp, i64]
    L.iem_kkt_residual.argtypes = [vp, vp, vp, dbl, vp, dbl, dbl, vp, vp, vp, vp]
    L.iem_kkt_solve_refined.argtypes = [vp, vp, vp, dbl, vp, dbl, dbl, vp, vp, i32, vp]
    L.iem_kkt_assemble_diag.argtypes = [vp, vp, vp, vp, vp, dbl, dbl]
    L.iem_kkt_residual_diag.argtypes = [vp, vp, vp, dbl, vp, vp, dbl, dbl, i32, vp, i64, vp, i64, vp, i64, vp]
    L.iem_kkt_solve_refined_diag.argtypes = [vp, vp, vp, dbl, vp, vp, dbl, dbl, i32, vp, i64, vp, i64, i32, vp]
    L.iem_kkt_diag_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_kkt_border_factor.argtypes = [vp, i64, i32, i32, vp, vp, vp, vp, vp, dbl]
    L.iem_kkt_border_solve.argtypes = [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp]
    L.iem_kkt_border_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_kkt_set_border.argtypes = [vp, i32]
    L.iem_kkt_factor_async.argtypes = [vp, vp]
    L.iem_barrier_create.argtypes = [vp, vp, vp, vp, vp, dbl, C.POINTER(vp)]
    L.iem_barrier_analyse.argtypes = [i64, i64, vp, vp, vp, vp, dbl, vp, vp, C.POINTER(BarrierInfo)]
    L.iem_barrier_destroy.argtypes = [vp]
    L.iem_barrier_info.argtypes = [vp, C.POINTER(BarrierInfo)]
    L.iem_barrier_start.argtypes = [vp] + [vp] * 7 + [dbl, dbl]
    L.iem_barrier_terms.argtypes = [vp] + [vp] * 9 + [dbl, vp, vp, vp]
    L.iem_barrier_step.argtypes = [vp] + [vp] * 8 + [dbl, dbl] + [vp] * 6
    L.iem_barrier_update.argtypes = [vp] + [vp] * 14 + [dbl, dbl]
    L.iem_barrier_error.argtypes = [vp] + [vp] * 9 + [dbl, vp]
    L.iem_barrier_merit.argtypes = [vp, vp, vp, vp, vp]
    L.iem_barrier_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_search_create.argtypes = [vp, C.POINTER(SearchOpts), C.POINTER(vp)]
    L.iem_search_destroy.argtypes = [vp]
    L.iem_search_reset.argtypes = [vp]
    L.iem_search_begin.argtypes = [vp] + [vp] * 8 + [dbl, dbl]
    L.iem_search_trial.argtypes = [vp] + [vp] * 6
    L.iem_search_accept.argtypes = [vp, vp, vp, dbl, dbl, vp]
    L.iem_search_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.iem_search_state.argtypes = [vp, C.POINTER(SearchState)]
    L.iem_search_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_soc_create.argtypes = [vp, C.POINTER(SocOpts), C.POINTER(vp)]
    L.iem_soc_destroy.argtypes = [vp]
    L.iem_soc_open.argtypes = [vp]
    L.iem_soc_rhs.argtypes = [vp] + [vp] * 8 + [dbl, vp]
    L.iem_soc_trial.argtypes = [vp] + [vp] * 7
    L.iem_soc_accept.argtypes = [vp, vp, vp, vp, dbl, dbl, vp]
    L.iem_soc_select.argtypes = [vp] + [vp] * 12
    L.iem_soc_device.argtypes = [vp, C.POINTER(vp)]
    L.iem_soc_state.argtypes = [vp, C.POINTER(SocState)]
    L.iem_soc_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_resto_create.argtypes = [vp, C.POINTER(RestoOpts), C.POINTER(vp)]
    L.iem_resto_destroy.argtypes = [vp]
    L.iem_resto_search.argtypes = [vp, C.POINTER(vp)]
    L.iem_resto_enter.argtypes = [vp] + [vp] * 8 + [dbl]
    L.iem_resto_terms.argtypes = [vp] + [vp] * 9 + [dbl, dbl] + [vp] * 3
    L.iem_resto_step.argtypes = [vp] + [vp] * 8 + [dbl, dbl, dbl] + [vp] * 6
    L.iem_resto_merit.argtypes = [vp, i32, vp, vp, vp, dbl, vp]
    L.iem_resto_begin.argtypes = [vp] + [vp] * 6 + [dbl, dbl]
    L.iem_resto_trial.argtypes = [vp] + [vp] * 6
    L.iem_resto_update.argtypes = [vp] + [vp] * 14 + [dbl, dbl]
    L.iem_resto_error.argtypes = [vp] + [vp] * 9 + [dbl, dbl, vp]
    L.iem_resto_check.argtypes = [vp, vp, vp, dbl]
    L.iem_resto_leave.argtypes = [vp] + [vp] * 5
    L.iem_resto_device.argtypes = [vp] + [C.POINTER(vp)] * 5
    L.iem_resto_state.argtypes = [vp, C.POINTER(RestoState)]
    L.iem_resto_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_mu_create.argtypes = [vp, C.POINTER(MuOpts), C.POINTER(vp)]
    L.iem_mu_destroy.argtypes = [vp]
    L.iem_mu_reset.argtypes = [vp, dbl]
    L.iem_mu_error.argtypes = [vp] + [vp] * 9 + [vp]
    L.iem_mu_update.argtypes = [vp, vp, vp]
    L.iem_mu_device.argtypes = [vp, C.POINTER(vp)]
    L.iem_mu_state.argtypes = [vp, C.POINTER(MuState)]
    L.iem_barrier_bind_mu.argtypes = [vp, vp]
    L.iem_search_bind_mu.argtypes = [vp, vp]
    L.iem_soc_bind_mu.argtypes = [vp, vp]
    L.iem_mu_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_barrier_mu_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_amu_create.argtypes = [vp, C.POINTER(AmuOpts), C.POINTER(vp)]
    L.iem_amu_destroy.argtypes = [vp]
    L.iem_amu_reset.argtypes = [vp]
    L.iem_amu_probe.argtypes = [vp] + [vp] * 6 + [vp] * 6 + [vp, vp]
    L.iem_amu_update.argtypes = [vp, vp, vp, i32, vp]
    L.iem_amu_device.argtypes = [vp, C.POINTER(vp)]
    L.iem_amu_state.argtypes = [vp, C.POINTER(MuState), C.POINTER(AmuState)]
    L.iem_amu_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_qf_create.argtypes = [vp, C.POINTER(QfOpts), C.POINTER(vp)]
    L.iem_qf_destroy.argtypes = [vp]
    L.iem_qf_reset.argtypes = [vp]
    L.iem_qf_begin.argtypes = [vp] + [vp] * 7 + [vp, vp, vp]
    L.iem_qf_alpha.argtypes = [vp] + [vp] * 6 + [vp] * 6 + [vp] * 6
    L.iem_qf_value.argtypes = [vp] + [vp] * 6 + [vp] * 6 + [vp] * 6
    L.iem_qf_update.argtypes = [vp, vp, i32, vp]
    L.iem_qf_device.argtypes = [vp, C.POINTER(vp)]
    L.iem_qf_state.argtypes = [vp, C.POINTER(MuState), C.POINTER(AmuState), C.POINTER(QfState)]
    L.iem_qf_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_mpc_create.argtypes = [vp, C.POINTER(MpcOpts), C.POINTER(vp)]
    L.iem_mpc_destroy.argtypes = [vp]
    L.iem_mpc_reset.argtypes = [vp]
    L.iem_mpc_bind_mu.argtypes = [vp, vp]
    L.iem_mpc_terms.argtypes = [vp] + [vp] * 7 + [vp, vp] + [vp] * 6 + [dbl, vp, i64]
    L.iem_mpc_step.argtypes = [vp] + [vp] * 7 + [vp] * 6 + [vp, dbl, dbl] + [vp] * 5 + [vp]
    L.iem_mpc_select.argtypes = [vp, vp, vp] + [vp] * 6 + [vp] * 6 + [vp]
    L.iem_mpc_device.argtypes = [vp, C.POINTER(vp)]
    L.iem_mpc_state.argtypes = [vp, C.POINTER(MpcState)]
    L.iem_mpc_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_init_create.argtypes = [vp, C.POINTER(InitOpts), C.POINTER(vp)]
    L.iem_init_destroy.argtypes = [vp]
    L.iem_init_reset.argtypes = [vp]
    L.iem_init_ls_terms.argtypes = [vp] + [vp] * 5 + [vp] + [vp] * 3
    L.iem_init_ls_apply.argtypes = [vp, vp, vp]
    L.iem_init_warm.argtypes = [vp] + [vp] * 7
    L.iem_init_mu.argtypes = [vp, vp, vp]
    L.iem_init_device.argtypes = [vp, C.POINTER(vp)]
    L.iem_init_state.argtypes = [vp, C.POINTER(InitState)]
    L.iem_init_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_conv_create.argtypes = [vp, C.POINTER(ConvOpts), C.POINTER(vp)]
    L.iem_conv_destroy.argtypes = [vp]
    L.iem_conv_reset.argtypes = [vp]
    L.iem_conv_check.argtypes = [vp, vp, vp, vp]
    L.iem_conv_keep.argtypes = [vp] + [vp] * 7
    L.iem_conv_restore.argtypes = [vp] + [vp] * 7
    L.iem_conv_step.argtypes = [vp, vp, vp, vp, vp]
    L.iem_conv_kept.argtypes = [vp] + [C.POINTER(vp)] * 7
    L.iem_conv_device.argtypes = [vp, C.POINTER(vp)]
    L.iem_conv_state.argtypes = [vp, C.POINTER(ConvState)]
    L.iem_conv_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_rmu_create.argtypes = [vp, vp, C.POINTER(RmuOpts), C.POINTER(vp)]
    L.iem_rmu_destroy.argtypes = [vp]
    L.iem_rmu_mu.argtypes = [vp, C.POINTER(vp)]
    L.iem_rmu_enter.argtypes = [vp, vp, dbl]
    L.iem_rmu_error.argtypes = [vp] + [vp] * 9 + [vp]
    L.iem_rmu_update.argtypes = [vp, vp]
    L.iem_rmu_trigger.argtypes = [vp, i32, vp]
    L.iem_rmu_device.argtypes = [vp, C.POINTER(vp)]
    L.iem_rmu_state.argtypes = [vp, C.POINTER(RmuState)]
    L.iem_resto_bind_mu.argtypes = [vp, vp]
    L.iem_rmu_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_resto_mu_source.argtypes = [C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_emit_source.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_emit_source.restype = i32
    L.iem_fixed_source.argtypes = [i32, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.iem_free.argtypes = [vp]
    L.iem_set_option.argtypes = [C.c_char_p, i64]
    L.iem_time_kernels.argtypes = [vp, vp, vp, vp, vp, i32, C.POINTER(dbl), C.POINTER(dbl)]
    L.iem_tuner_choice.argtypes = [vp, i32, vp, C.POINTER(i32)]
    L.iem_tune.argtypes = [vp, vp, vp, dbl, vp, vp]
    _lib = L
    return L


def check(rc: int):
    if rc != 0:
        raise IemError(f"libiem_hip error {rc}: {lib().iem_last_error().decode(errors='replace')}")


def set_option(name: str, value: int):
    check(lib().iem_set_option(name.encode(), int(value)))


# generator knobs and their defaults (csrc/iem_codegen.hpp: struct Options)
OPTION_DEFAULTS = dict(store_mode=2, nt_stores=1, block=0, lds_slots=24, reorder=1, no_fuse=0, hess_merge=0, ablate=0,
                       min_waves=0, fp_contract=0, fuse_zero=1, fuse_groups=1, split_small=64, poll_obj=1, xcd_remap=0, overlap=1, wide_stores=1, obj_wgs=1024, det_shared=1, flat2d=0, flush32=2, autotune=0, autotune_min_blocks=400, pull_scatter=1, fold_colloc=2, fold_max_n=6, det_axis=1, det_scatter=1, det_scatter_max=1 << 28, lazy_loads=2, lazy_min_loads=48, lazy_all_kinds=0, name_tag=0,
                       big_batch_slots=48, big_batch_jac=4000, big_batch_hess=4000, big_xcd=1, big_tile=1024, pair_kernel=1, store_wait=0, comm_timeout_ms=5000,
                       carrier=0, two_sided=0, phase_kernels=1, jac_split=1, cons_direct_2d=1, digit_fields=1, param_kinds=0, scaled_kinds=0, kkt_kinds=0,
                       scaled_phase_kinds=0)


def option_array(opts: dict):
    """``iem_option_t[]`` for ``iem_create_opts`` (per-handle generator options)."""
    unknown = set(opts) - set(OPTION_DEFAULTS)
    if unknown:
        raise KeyError(f"unknown generator option(s): {sorted(unknown)}")
    arr = (Option * max(1, len(opts)))()
    for i, (k, v) in enumerate(opts.items()):
        arr[i].name = k.encode()
        arr[i].value = int(v)
    return arr, len(opts)


class options:
    """``with options(split_small=0): ...`` — PROCESS DEFAULTS of the generator knobs for the models
    created inside the block, restored on exit.  One model only: ``ExaModel(core, options={...})``
    (``iem_create_opts``), which leaves the defaults alone."""

    def __init__(self, **kw):
        unknown = set(kw) - set(OPTION_DEFAULTS)
        if unknown:
            raise KeyError(f"unknown generator option(s): {sorted(unknown)}")
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            set_option(k, OPTION_DEFAULTS[k])
        return False


def _source(fn, *args):
    """``(text, key)`` of a source entry point: ``fn(*args, &text, &key)``, the text decoded and freed."""
    p, key = C.c_void_p(), C.c_uint64()
    check(fn(*args, C.byref(p), C.byref(key)))
    try:
        return C.string_at(p).decode(), int(key.value)
    finally:
        lib().iem_free(p)


def emit_source(blob: bytes):
    """Generated HIP source of a model and its cache key (no device needed)."""
    return _source(lib().iem_emit_source, blob, len(blob))


def kkt_analyse_blob(blob: bytes, group: int = 0):
    """Host analysis of the chain KKT solver behind ``iem_kkt_create`` (no device): ``(info dict, blk, loc, rows, cols, dest, seg,
    perm)`` as numpy arrays."""
    import numpy as np
    L = lib()
    info = KktInfo()
    ptrs = [C.c_void_p() for _ in range(7)]
    nd, npm = C.c_int64(), C.c_int64()
    check(L.iem_kkt_analyse_blob(blob, len(blob), int(group), C.byref(info), *[C.byref(p) for p in ptrs], C.byref(nd), C.byref(npm)))
    n = int(info.n)
    shapes = [(n, np.int64), (n, np.int64), (int(info.nc), np.int32), (int(info.nc), np.int32), (nd.value, np.int64), (nd.value + 1, np.uint32), (npm.value, np.uint32)]
    out = []
    try:
        for p, (cnt, dt) in zip(ptrs, shapes):
            out.append(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int64 if dt == np.int64 else C.c_int32 if dt == np.int32 else C.c_uint32)), shape=(max(cnt, 1),))[:cnt].copy())
    finally:
        for p in ptrs:
            L.iem_free(p)
    return ({k: int(getattr(info, k)) for k, _ in KktInfo._fields_}, *out)


def kkt_source(nb: int, ne: int, nc: int = 12):
    """HIP source of the chain KKT solver's kernels for block size ``nb`` / border size ``ne`` / coupling width ``nc`` and its
    cache key."""
    return _source(lib().iem_kkt_source, int(nb), int(ne), int(nc))


def kkt_diag_source():
    """HIP source of the KKT object's own kernels (``kkt_gather_d`` / ``kkt_residual_dm`` / ``kkt_axpy_m``: ``iem_kkt_assemble*``,
    ``iem_kkt_residual*``, ``iem_kkt_solve_refined*``) and its cache key."""
    return _source(lib().iem_kkt_diag_source)


def kkt_border_source():
    """HIP source of the dense border's kernels (``kkt_border_ldl`` / ``kkt_border_solve``) and its cache key."""
    return _source(lib().iem_kkt_border_source)


def barrier_source():
    """HIP source of the interior-point barrier layer's kernels (``barrier_start`` / ``_terms`` / ``_step`` / ``_update`` / ``_error`` /
    ``_merit``: the ``iem_barrier_*`` calls) and its cache key."""
    return _source(lib().iem_barrier_source)


def search_source():
    """HIP source of the filter line search's kernels (``search_begin`` / ``search_trial`` / ``search_accept``: the ``iem_search_*``
    calls) and its cache key.  A code object of its own: not one of :func:`fixed_sources`."""
    return _source(lib().iem_search_source)


def soc_source():
    """HIP source of the second-order correction's kernels (``soc_open`` / ``soc_rhs`` / ``soc_trial`` / ``soc_accept`` /
    ``soc_select``: the ``iem_soc_*`` calls) and its cache key.  A code object of its own: not one of :func:`fixed_sources`."""
    return _source(lib().iem_soc_source)


def resto_source():
    """HIP source of the feasibility restoration phase's kernels (``resto_enter`` ... ``resto_leave``: the ``iem_resto_*`` calls) and
    its cache key.  A code object of its own: not one of :func:`fixed_sources`."""
    return _source(lib().iem_resto_source)


def mu_source():
    """HIP source of the barrier parameter's kernels (``mu_error`` / ``mu_update`` / ``mu_reset``: the ``iem_mu_*`` calls) and its cache
    key.  A code object of its own: not one of :func:`fixed_sources`."""
    return _source(lib().iem_mu_source)


def amu_source():
    """HIP source of the adaptive barrier parameter's kernels (``amu_probe`` / ``amu_update`` / ``amu_reset``: the ``iem_amu_*`` calls) and
    its cache key.  A code object of its own: not one of :func:`fixed_sources`."""
    return _source(lib().iem_amu_source)


def qf_source():
    """HIP source of the quality-function oracle's kernels (``qf_begin`` / ``qf_alpha`` / ``qf_value`` / ``qf_update`` / ``qf_reset``: the
    ``iem_qf_*`` calls) and its cache key.  A code object of its own: not one of :func:`fixed_sources`."""
    return _source(lib().iem_qf_source)


def mpc_source():
    """HIP source of Mehrotra's corrector's kernels (``mpc_terms`` / ``mpc_step`` / ``mpc_select`` / ``mpc_reset``: the ``iem_mpc_*``
    calls) and its cache key.  A code object of its own: not one of :func:`fixed_sources`."""
    return _source(lib().iem_mpc_source)


def init_source():
    """HIP source of the starting point's kernels (``init_ls_terms`` / ``init_ls_norm`` / ``init_ls_apply`` / ``init_warm`` /
    ``init_mu`` / ``init_reset``: the ``iem_init_*`` calls) and its cache key.  A code object of its own: not one of
    :func:`fixed_sources`."""
    return _source(lib().iem_init_source)


def conv_source():
    """HIP source of the stopping test's kernels (``conv_xmax`` / ``conv_decide`` / ``conv_stepmax`` / ``conv_step_decide`` /
    ``conv_keep`` / ``conv_restore`` / ``conv_reset``: the ``iem_conv_*`` calls) and its cache key.  A code object of its own: not
    one of :func:`fixed_sources`."""
    return _source(lib().iem_conv_source)


def rmu_source():
    """HIP source of the restoration parameter's kernels (``rmu_error`` / ``rmu_enter`` / ``rmu_update`` / ``rmu_trigger`` /
    ``rmu_gather``: the ``iem_rmu_*`` calls) and its cache key.  A code object of its own: not one of :func:`fixed_sources`."""
    return _source(lib().iem_rmu_source)


def resto_mu_source():
    """HIP source of the BOUND variant of the restoration kernels (``iem_resto_bind_mu``: the text of :func:`resto_source` with ``mu``,
    ``tau`` and ``zeta`` read from the restoration block) and its cache key.  A code object of its own: not one of :func:`fixed_sources`."""
    return _source(lib().iem_resto_mu_source)


def barrier_mu_source():
    """HIP source of the BOUND variant of the barrier layer's kernels (``iem_barrier_bind_mu``: the text of :func:`barrier_source` with
    ``mu`` and ``tau`` read from an ``iem_mu`` block) and its cache key.  A code object of its own: not one of :func:`fixed_sources`."""
    return _source(lib().iem_barrier_mu_source)


def fixed_sources():
    """``(name, src, key)`` of every hand-written code object whose source depends on no model and no shape (``iem_fixed_source``):
    the four above, and whatever the library gains."""
    L, i, name = lib(), 0, C.c_char_p()
    while L.iem_fixed_source(i, None, None, None) != IEM_E_ARG:      # (IEM_E_ARG: past the end; any other failure is raised below)
        src, key = _source(L.iem_fixed_source, i, C.byref(name))
        yield name.value.decode(), src, key
        i += 1


def barrier_analyse(lvar, uvar, lcon, ucon, relax: float = 1e-8):
    """The host analysis of ``iem_barrier_create`` (no device): ``(dict(xl, xu, rl, ru, ceq), fx, fc, info dict)`` as numpy arrays —
    relaxed bounds, presence flags (bit 0 lower, bit 1 upper, bit 2 equality row) and the counts of ``iem_barrier_info``."""
    import numpy as np
    lvar, uvar, lcon, ucon = (np.ascontiguousarray(a, dtype=np.float64) for a in (lvar, uvar, lcon, ucon))
    n, m = len(lvar), len(lcon)
    if len(uvar) != n or len(ucon) != m:
        raise ValueError("lvar / uvar and lcon / ucon must have equal lengths")
    bounds, flags = np.zeros(max(2 * n + 3 * m, 1)), np.zeros(max(n + m, 1), dtype=np.uint8)
    info = BarrierInfo()
    info.struct_size = C.sizeof(BarrierInfo)
    check(lib().iem_barrier_analyse(n, m, lvar.ctypes.data, uvar.ctypes.data, lcon.ctypes.data, ucon.ctypes.data, float(relax), bounds.ctypes.data,
                                    flags.ctypes.data, C.byref(info)))
    parts = dict(xl=bounds[:n], xu=bounds[n:2 * n], rl=bounds[2 * n:2 * n + m], ru=bounds[2 * n + m:2 * n + 2 * m], ceq=bounds[2 * n + 2 * m:2 * n + 3 * m])
    return parts, flags[:n], flags[n:n + m], {k: int(getattr(info, k)) for k, _ in BarrierInfo._fields_ if k != "struct_size"}


def kkt_many_width(nb: int, ne: int, nc: int = 12) -> int:
    """Columns per chunk of the multi-column solves for that shape (``KKT_MR`` of its source)."""
    import re
    return int(re.search(r"^#define KKT_MR (\d+)$", kkt_source(nb, ne, nc)[0], re.M).group(1))


def precompile_source(src: str, key: int, arch: str = "gfx950", defer: list = None, force: bool = False) -> str:
    """Offline-compile a complete HIP source (first line ``// iem-flags: ...``) into the in-tree code-object cache
    (``hipcc --genco --offload-arch=gfx950``); returns the ``.hsaco`` path.  With ``defer`` (a list) the hipcc command
    is appended to the list instead of being run: ``run_deferred`` compiles them in parallel."""
    first = src.split("\n", 1)[0]
    assert first.startswith("// iem-flags:"), first
    os.makedirs(KERNEL_DIR, exist_ok=True)
    out = os.path.join(KERNEL_DIR, f"iem_{key:016x}.hsaco")
    if os.path.exists(out) and not force:
        return out
    hip = os.path.join(KERNEL_DIR, f"iem_{key:016x}.hip")
    with open(hip, "w") as f:
        f.write(src)
    flags = first[len("// iem-flags:"):].split()
    cmd = [os.path.join(ROCM, "bin", "hipcc"), "--genco", f"--offload-arch={arch}", *flags, "-o", out + ".tmp", hip]
    if defer is not None:
        if not any(c[1] == out for c in defer):
            defer.append((cmd, out))
        return out
    subprocess.check_call(cmd)
    os.replace(out + ".tmp", out)
    return out


def emit_launch_plan(blob: bytes) -> str:
    L = lib()
    L.iem_emit_launch_plan.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
    p = C.c_void_p()
    check(L.iem_emit_launch_plan(blob, len(blob), C.byref(p)))
    try:
        return C.string_at(p).decode()
    finally:
        L.iem_free(p)


def blob_array(blob: bytes, array_id: int):
    """Model array `array_id` as the library holds it after parsing (float64), including arrays it
    synthesised itself (lattice recovery).  Tooling/tests."""
    import numpy as np
    L = lib()
    L.iem_blob_array.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    p, n = C.c_void_p(), C.c_int64()
    check(L.iem_blob_array(blob, len(blob), int(array_id), C.byref(p), C.byref(n)))
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(max(n.value, 1),))[:n.value].copy()
    finally:
        L.iem_free(p)


def blob_hess_structure(blob: bytes, base: int = 0):
    """Hessian structure of a blob under the current options (host computation, no device)."""
    import numpy as np
    L = lib()
    L.iem_blob_hess_structure.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_int64)]
    r, c, n = C.c_void_p(), C.c_void_p(), C.c_int64()
    check(L.iem_blob_hess_structure(blob, len(blob), base, C.byref(r), C.byref(c), C.byref(n)))
    try:
        rows = np.ctypeslib.as_array(C.cast(r, C.POINTER(C.c_int64)), shape=(max(n.value, 1),))[:n.value].copy()
        cols = np.ctypeslib.as_array(C.cast(c, C.POINTER(C.c_int64)), shape=(max(n.value, 1),))[:n.value].copy()
    finally:
        L.iem_free(r)
        L.iem_free(c)
    return rows, cols


def blob_param_coord_structure(blob: bytes, which: int, base: int = 0):
    """Structure of one explicit θ block of a blob (host computation, no device): ``which`` = 0 ``∂c/∂θ``, 1 ``∂²L/∂x∂θ``,
    2 ``∂²L/∂θ²`` — what ``ExaModel.jacp_structure`` / ``hessxp_structure`` / ``hesspp_structure`` report."""
    import numpy as np
    L = lib()
    L.iem_blob_param_coord_structure.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                 C.POINTER(C.c_int64)]
    r, c, n = C.c_void_p(), C.c_void_p(), C.c_int64()
    check(L.iem_blob_param_coord_structure(blob, len(blob), int(which), int(base), C.byref(r), C.byref(c), C.byref(n)))
    try:
        rows = np.ctypeslib.as_array(C.cast(r, C.POINTER(C.c_int64)), shape=(max(n.value, 1),))[:n.value].copy()
        cols = np.ctypeslib.as_array(C.cast(c, C.POINTER(C.c_int64)), shape=(max(n.value, 1),))[:n.value].copy()
    finally:
        L.iem_free(r)
        L.iem_free(c)
    return rows, cols


def blob_has_folded_runs(blob: bytes) -> bool:
    """Does a template of ``blob`` fold several parameter groups into one box axis (its grid hint holds a
    virtual run id, ``items.RUN_GRID_LO`` ..)?  Such a model cannot be sharded or chained."""
    import numpy as np
    from .items import RUN_GRID_LO, RUN_GRID_HI
    w = np.frombuffer(blob, dtype=np.int64)
    n_tpl, n_arr = int(w[5]), int(w[6])
    for off in w[14 + 6 * n_arr:14 + 6 * n_arr + n_tpl]:
        nd, g = int(w[off + 2]), int(w[off + 6])
        for _ in range(nd if g > 0 else 0):
            if RUN_GRID_LO <= g % 4096 - 1 < RUN_GRID_HI:
                return True
            g //= 4096
    return False


def shard_blob(blob: bytes, group: int, rank: int, world: int):
    """``iem_shard_blob``: rank ``rank``'s shard of a GLOBAL blob, cut in C++ without a device —
    ``(local blob, info dict, var_map, var_flag, [template dicts])``."""
    import numpy as np
    L = lib()
    ob, on, info = C.c_void_p(), C.c_size_t(), ShardT()
    vm, vf, tp, it = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    check(L.iem_shard_blob(blob, len(blob), group, rank, world, C.byref(ob), C.byref(on), C.byref(info),
                           C.byref(vm), C.byref(vf), C.byref(tp), C.byref(it)))
    try:
        local = C.string_at(ob, on.value)
        n = int(info.nvar)
        var_map = np.ctypeslib.as_array(C.cast(vm, C.POINTER(C.c_int64)), shape=(max(n, 1),))[:n].copy()
        var_flag = np.ctypeslib.as_array(C.cast(vf, C.POINTER(C.c_uint8)), shape=(max(n, 1),))[:n].copy()
        tarr = C.cast(tp, C.POINTER(ShardTemplate))
        n_items = sum(int(tarr[i].n_items) for i in range(int(info.n_templates)) if tarr[i].items_offset >= 0)
        items = np.ctypeslib.as_array(C.cast(it, C.POINTER(C.c_int64)), shape=(max(n_items, 1),))[:n_items].copy()
        tpl = [tarr[i].asdict(items) for i in range(int(info.n_templates))]
    finally:
        for p in (ob, vm, vf, tp, it):
            L.iem_free(p)
    d = info.asdict()
    # the back halo, as the flags tell it (iem_shard_t keeps its layout: halo / halo_reach / halo_doubles are the front one)
    d["halo_right_vars"] = int(((var_flag & 8) != 0).sum())
    return local, d, var_map, var_flag, tpl


def precompile(blob: bytes, arch: str = "gfx950", force: bool = False, defer: list = None) -> str:
    """``precompile_source`` of a model's kernels: the source is generated now — under the CURRENT generator options."""
    return precompile_source(*emit_source(blob), arch=arch, defer=defer, force=force)


def run_deferred(jobs: list, workers: int = 0) -> None:
    """Run the hipcc commands collected by ``precompile(..., defer=jobs)`` on a small thread pool."""
    from concurrent.futures import ThreadPoolExecutor

    def one(job):
        cmd, out = job
        subprocess.check_call(cmd)
        os.replace(out + ".tmp", out)
    workers = workers or max(1, min(6, len(os.sched_getaffinity(0)) - 1))
    with ThreadPoolExecutor(max_workers=workers) as ex:
        list(ex.map(one, jobs))
