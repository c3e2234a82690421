"""ctypes binding of include/fastbn.h and the reference-shaped Python classes."""
import atexit
import ctypes as C
import weakref
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FBN_LIB_PATH: an alternative build of the same library (A/B runs of build-time switches, tools/)
LIB_PATH = os.environ.get("FBN_LIB_PATH") or os.path.join(_HERE, "libfastbn.so")

_vp, _i32, _i64, _dbl, _cstr = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_char_p
_pp = C.POINTER(C.c_void_p)

# name -> argtypes (all functions return int status except fbn_last_error)
_SIGS = {
    "fbn_version": [_vp, _vp],
    "fbn_device_count": [_vp],
    "fbn_network_load_xmlbif": [_cstr, _pp],
    "fbn_network_create": [C.c_int, _vp, _vp, _vp, _vp, _vp, _pp],
    "fbn_network_node_counts": [_vp, C.c_int, _vp, _vp, _vp, _vp],
    "fbn_network_create_cpt": [C.c_int, _vp, _vp, _vp, _vp, _vp, _pp],
    "fbn_network_node_probs": [_vp, C.c_int, _vp, _vp, _vp, _vp],
    "fbn_network_num_nodes": [_vp, _vp],
    "fbn_network_dims": [_vp, _vp],
    "fbn_network_name": [_vp, C.c_int, C.c_char_p, C.c_int],
    "fbn_network_destroy": [_vp],
    "fbn_evidence_load_libsvm": [_cstr, C.c_int, _vp, _vp, _i64, _vp],
    "fbn_dataset_load_csv": [_cstr, _pp],
    "fbn_synth_forward_sample": [_vp, _i64, C.c_uint64, _vp],
    "fbn_synth_evidence": [_vp, _i64, C.c_int, C.c_uint64, C.c_int, _vp],
    "fbn_write_csv": [_cstr, _vp, C.c_int, _i64, _vp],
    "fbn_write_libsvm": [_cstr, _vp, _i64, C.c_int, _vp],
    "fbn_dataset_shape": [_vp, _vp, _vp],
    "fbn_dataset_dims": [_vp, _vp],
    "fbn_dataset_columns": [_vp, _vp],
    "fbn_dataset_var_name": [_vp, C.c_int, C.c_char_p, C.c_int],
    "fbn_dataset_destroy": [_vp],
    "fbn_jt_plan_create": [_vp, C.c_int, _pp],
    "fbn_jt_forest_plan_create": [_vp, C.c_int, _pp],
    "fbn_jt_plan_components": [_vp, _vp, _vp],
    "fbn_jt_plan_info_get": [_vp, _vp],
    "fbn_jt_plan_dump": [_vp, _cstr, _cstr],
    "fbn_jt_run": [_vp, _vp, _i64, _vp, _vp, _vp],
    "fbn_jt_run_device": [_vp, _vp, _i64, _vp, _vp, _vp],
    "fbn_jt_evidence_validate": [_vp, _vp, _i64, _vp],
    "fbn_jt_set_evidence_check": [_vp, C.c_int],
    "fbn_jt_set_kernel_timing": [_vp, C.c_int],
    "fbn_jt_score": [_vp, _vp, _vp, _i64, _vp, _vp],
    "fbn_jt_set_output_layout": [_vp, C.c_int],
    "fbn_jt_score_terms_device": [_vp, _vp, _vp, _i64, _vp, _vp],
    "fbn_jt_last_kernel_ms": [_vp, _vp],
    "fbn_jt_stream_schedule": [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp],
    "fbn_jt_set_waves_per_cu": [_vp, C.c_int],
    "fbn_jt_set_variant": [_vp, C.c_int],
    "fbn_jt_debug_op_cycles": [_vp, C.c_int, _vp],
    "fbn_jt_kernel_source": [_vp, C.c_char_p, C.c_int64, _vp],
    "fbn_jt_kernel_cache_path": [_vp, C.c_char_p, C.c_int64],
    "fbn_jt_kernel_options": [C.c_char_p, C.c_int64],
    "fbn_jt_kernel_build": [_vp],
    "fbn_jt_kernel_placement": [_vp, _vp],
    "fbn_jt_debug_force_fixup": [_vp, C.c_int],
    "fbn_jt_debug_flagged_blocks": [_vp, _vp],
    "fbn_jt_set_exact": [_vp, C.c_int],
    "fbn_jt_plan_destroy": [_vp],
    "fbn_ci_dataset_upload": [_vp, C.c_int, _i64, _vp, C.c_int, _pp],
    "fbn_ci_dataset_from_device": [_vp, C.c_int, _i64, _vp, C.c_int, _pp],
    "fbn_ci_set_kernel_timing": [_vp, C.c_int],
    "fbn_ci_run": [_vp, _vp, _i64, C.c_int, _dbl, _vp, _vp, _vp, _vp, _vp],
    "fbn_ci_counts": [_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _i64, _vp],
    "fbn_ci_last_kernel_ms": [_vp, _vp],
    "fbn_ci_decision_margin": [_vp, _vp, _vp, C.c_int],
    "fbn_ci_debug_counts": [_vp, _vp, _i64, C.c_int, _vp, _i64],
    "fbn_ci_level0_info": [_vp, _vp],
    "fbn_ci_debug_level0_range": [_vp, _i64, _i64, _vp],
    "fbn_pc_decision_margin": [_vp, _vp, _vp],
    "fbn_ci_ctx_destroy": [_vp],
    "fbn_pc_stable": [_vp, _dbl, C.c_int, C.c_int, _pp],
    "fbn_pc_num_levels": [_vp, _vp],
    "fbn_pc_level_tests": [_vp, _vp],
    "fbn_pc_level_launched": [_vp, _vp],
    "fbn_pc_num_edges": [_vp, _vp],
    "fbn_pc_edges": [_vp, _vp],
    "fbn_pc_sepsets": [_vp, _vp, _i64, _vp],
    "fbn_pc_timing": [_vp, _vp, _vp],
    "fbn_pc_path": [_vp, _vp],
    "fbn_jt_tile_program": [_vp, _vp, _vp, _vp, _vp],
    "fbn_pc_result_record": [_vp, _vp, C.c_int64, _vp],
    "fbn_pc_small_eligible": [_vp, C.c_int, _vp],
    "fbn_pc_small_eligible_shape": [C.c_int, C.c_int64, _vp, C.c_int, _vp],
    "fbn_pc_device_bytes": [_vp, _vp],
    "fbn_pc_orient_skeleton": [C.c_int, _vp, C.c_int, _vp, C.c_int64, _vp],
    "fbn_pc_level": [_vp, C.c_double, C.c_int, C.c_int, _vp, C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp],
    "fbn_pc_num_oriented_edges": [_vp, _vp],
    "fbn_pc_oriented_edges": [_vp, _vp],
    "fbn_pc_shd_bif": [_vp, C.c_char_p, _vp],
    "fbn_shd_bif": [C.c_char_p, C.c_int, _vp, C.c_int, _vp],
    "fbn_pc_result_destroy": [_vp],
    "fbn_pc_dist_create": [C.c_int, _dbl, C.c_int, C.c_int, _pp],
    "fbn_pc_dist_level": [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp],
    "fbn_pc_dist_num_edges": [_vp, _vp],
    "fbn_pc_dist_edges": [_vp, _vp, _i64],
    "fbn_pc_dist_run": [_vp, _vp, _vp],
    "fbn_pc_dist_pack": [_vp, _vp, _vp, _i64, _i64, _vp],
    "fbn_pc_dist_pairs_chunk": [_vp, _vp],
    "fbn_pc_dist_pairs_export": [_vp, _vp, C.c_int],
    "fbn_pc_dist_pairs_import": [_vp, _vp, _vp, C.c_int],
    "fbn_pc_dist_apply": [_vp, _vp, _vp],
    "fbn_pc_dist_result": [_vp, _pp],
    "fbn_pc_dist_destroy": [_vp],
    "fbn_param_family_sizes": [C.c_int, _vp, _vp, _vp, _vp, _vp],
    "fbn_param_counts": [_vp, _vp, _vp, _vp, _i64, _vp],
    "fbn_param_learn": [_vp, _vp, _vp, _vp, _pp],
    "fbn_param_set_tuning": [_vp, _i64, _i64],
    "fbn_pdag_to_dag": [C.c_int, _vp, C.c_int, _vp, _vp],
    "fbn_sampler_create": [_vp, C.c_int, _pp],
    "fbn_sampler_destroy": [_vp],
    "fbn_sample_forward": [_vp, _i64, C.c_uint64, _vp],
    "fbn_sample_forward_device": [_vp, _i64, C.c_uint64, _vp, _vp],
    "fbn_lw_run": [_vp, C.c_int, _vp, _i64, _i64, C.c_uint64, _i64, _vp, _vp, _vp],
    "fbn_lw_run_device": [_vp, C.c_int, _vp, _i64, _i64, C.c_uint64, _i64, _vp, _vp, _vp, _vp],
    "fbn_lw_debug_samples": [_vp, C.c_int, _vp, _i64, _i64, C.c_uint64, _i64, _vp, _vp, _vp],
    "fbn_sampler_last_kernel_ms": [_vp, _vp],
    "fbn_score_marginals": [_vp, _vp, _vp, _i64, _vp, _vp],
    "fbn_lbp_create": [_vp, C.c_int, _pp],
    "fbn_lbp_destroy": [_vp],
    "fbn_lbp_info": [_vp, _vp, _vp, _vp, _vp],
    "fbn_lbp_run": [_vp, _vp, _i64, C.c_int, _dbl, _dbl, _vp, _vp, _vp],
    "fbn_lbp_run_device": [_vp, _vp, _i64, C.c_int, _dbl, _dbl, _vp, _vp, _vp, _vp],
    "fbn_lbp_debug_messages": [_vp, _vp, _i64, C.c_int, _dbl, _vp],
    "fbn_lbp_set_tuning": [_vp, _i64, C.c_int],
    "fbn_lbp_last_kernel_ms": [_vp, _vp],
    "fbn_epis_create": [_vp, C.c_int, _pp],
    "fbn_epis_destroy": [_vp],
    "fbn_epis_run": [_vp, _vp, _i64, _i64, C.c_uint64, _i64, C.c_int, _dbl, _dbl, _dbl, _vp, _vp, _vp],
    "fbn_epis_run_device": [_vp, _vp, _i64, _i64, C.c_uint64, _i64, C.c_int, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp],
    "fbn_epis_debug_samples": [_vp, _vp, _i64, _i64, C.c_uint64, _i64, C.c_int, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp],
    "fbn_epis_set_tuning": [_vp, _i64],
    "fbn_epis_info": [_vp, _vp, _vp],
    "fbn_epis_last_kernel_ms": [_vp, _vp, _vp],
    "fbn_ais_create": [_vp, C.c_int, _pp],
    "fbn_ais_destroy": [_vp],
    "fbn_ais_run": [_vp, C.c_int, _vp, _i64, _i64, _i64, _i64, C.c_uint64, _i64, _dbl, _vp, _vp, _vp],
    "fbn_ais_run_device": [_vp, C.c_int, _vp, _i64, _i64, _i64, _i64, C.c_uint64, _i64, _dbl, _vp, _vp, _vp, _vp],
    "fbn_ais_debug_samples": [_vp, C.c_int, _vp, _i64, _i64, _i64, _i64, C.c_uint64, _i64, _dbl, _vp, _vp, _vp, _vp],
    "fbn_ais_set_tuning": [_vp, _i64, C.c_int],
    "fbn_ais_info": [_vp, _i64, _vp, _vp, _vp, _vp],
    "fbn_ais_last_kernel_ms": [_vp, _vp],
    "fbn_ais_eta": [C.c_int, C.c_int, _vp],
    "fbn_mpe_create": [_vp, C.c_int, _pp],
    "fbn_mpe_destroy": [_vp],
    "fbn_mpe_info": [_vp, _vp, _vp, _vp, _vp],
    "fbn_mpe_run": [_vp, _vp, _i64, _vp, _vp],
    "fbn_mpe_run_device": [_vp, _vp, _i64, _vp, _vp, _vp],
    "fbn_mpe_debug_messages": [_vp, _vp, _i64, _vp, _vp],
    "fbn_mpe_set_tuning": [_vp, C.c_int, _i64],
    "fbn_mpe_last_kernel_ms": [_vp, _vp],
    "fbn_em_create": [_vp, C.c_int, _pp],
    "fbn_em_destroy": [_vp],
    "fbn_em_info": [_vp, _vp, _vp, _vp, _vp, _vp],
    "fbn_em_estep": [_vp, _vp, _i64, _vp, _vp],
    "fbn_em_estep_device": [_vp, _vp, _i64, _vp, _vp, _vp],
    "fbn_em_run": [_vp, _vp, _i64, C.c_int, _dbl, _dbl, _vp, _vp],
    "fbn_em_set_parameters": [_vp, _vp],
    "fbn_em_network": [_vp, _pp],
    "fbn_em_debug_posteriors": [_vp, _vp, _i64, _vp],
    "fbn_em_set_tuning": [_vp, C.c_int, _i64],
    "fbn_em_last_kernel_ms": [_vp, _vp],
    "fbn_hc_table_bytes": [_i64, _vp],
    "fbn_hc_penalty": [_cstr, _i64, _vp],
    "fbn_score_families": [_vp, _dbl, _i64, _vp, _vp, _vp, _vp],
    "fbn_score_families_host": [C.c_int, _vp, _vp, _i64, _dbl, _i64, _vp, _vp, _vp, _vp],
    "fbn_hc_set_tuning": [_vp, _i64],
    "fbn_hc_run": [_vp, _vp, _pp],
    "fbn_hc_run_host": [C.c_int, _vp, _vp, _i64, _vp, _pp],
    "fbn_hc_result_info": [_vp, _vp],
    "fbn_hc_result_parents": [_vp, _vp, _vp],
    "fbn_hc_result_node_scores": [_vp, _vp, _vp],
    "fbn_hc_result_trace": [_vp, _vp, _vp],
    "fbn_hc_result_destroy": [_vp],
}


class FastBNError(RuntimeError):
    pass


class _Lib:
    """Lazily loaded libfastbn.so.  Missing library => every call raises (no CPU fallback)."""

    def __init__(self):
        self._h = None

    def load(self):
        if self._h is None:
            if not os.path.exists(LIB_PATH):
                raise FastBNError(f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback)")
            try:
                # torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's): load it first
                # so that one HIP runtime serves both when they share a process
                import torch  # noqa: F401
            except ImportError:
                pass
            h = C.CDLL(LIB_PATH)
            for name, args in _SIGS.items():
                f = getattr(h, name)
                f.argtypes = args
                f.restype = C.c_int
            h.fbn_last_error.restype = C.c_char_p
            h.fbn_last_error.argtypes = []
            self._h = h
        return self._h

    def __getattr__(self, name):
        h = self.load()
        f = getattr(h, name)
        if name == "fbn_last_error":
            return f

        def call(*args):
            rc = f(*args)
            if rc != 0:
                err = FastBNError(f"{name}: {h.fbn_last_error().decode()} (code {rc})")
                err.code = rc  # the fbn_err_t value (include/fastbn.h)
                raise err
            return rc

        return call


lib = _Lib()

# Every live handle (networks, datasets, plans, CI contexts, results, sessions) is destroyed by an
# atexit hook, before the interpreter's module teardown and before the HIP runtime's own exit
# handlers: no fbn_* destroy ever runs from a finalizer racing those (or after `lib` is gone).
# Destroy order: results and sessions, then plans and contexts (they drain their device work),
# then host-only handles.
_LIVE = weakref.WeakSet()
_CLOSE_ORDER = {"PCResult": 0, "PCDistSession": 1, "JunctionTree": 2, "Sampler": 2, "LikelihoodWeighting": 2,
                "LoopyBeliefPropagation": 2, "EPISBN": 2, "AISBN": 2, "SelfImportanceSampling": 2, "MostProbableExplanation": 2,
                "ExpectationMaximization": 2,
                "IndependenceTest": 3, "Dataset": 4, "Network": 5}


def _register(obj):
    _LIVE.add(obj)


def close_all():
    """Destroy every live handle now (also run at interpreter exit)."""
    objs = sorted(list(_LIVE), key=lambda o: _CLOSE_ORDER.get(type(o).__name__, 9))
    for o in objs:
        try:
            o.close()
        except Exception:  # noqa: BLE001 (exit path: keep closing the rest)
            pass


atexit.register(close_all)


class _Handle:
    """A libfastbn handle: `_h`, destroyed once by close() (explicitly, by __del__, or at exit)."""
    _destroy = None

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            getattr(lib, self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (finalizer)
            pass


def _p(a):
    return None if a is None else a.ctypes.data


def device_count():
    n = C.c_int(0)
    lib.fbn_device_count(C.byref(n))
    return n.value


class _PlanInfo(C.Structure):
    _fields_ = [("num_nodes", C.c_int32), ("num_cliques", C.c_int32), ("num_separators", C.c_int32),
                ("num_levels", C.c_int32), ("root", C.c_int32), ("sum_dom", C.c_int32),
                ("clique_entries", C.c_int64), ("separator_entries", C.c_int64),
                ("algorithmic_bytes_per_case", C.c_int64), ("num_ops", C.c_int32),
                ("max_vars_per_table", C.c_int32), ("specialized_eligible", C.c_int32),
                ("variant", C.c_int32), ("streamed_eligible", C.c_int32), ("streamed_waves", C.c_int32),
                ("streamed_split_efficiency", C.c_double), ("tiled_eligible", C.c_int32),
                ("tiled_passes", C.c_int32), ("tiled_entry_visits", C.c_int64), ("tiled_lds_bytes", C.c_int64),
                ("tiled_table_bytes", C.c_int64)]


class Network(_Handle):
    """Discrete BN loaded from XMLBIF (CustomNetwork::GetNetFromXMLBIFFile)."""

    _destroy = "fbn_network_destroy"

    def __init__(self, path=None, _handle=None):
        h = C.c_void_p() if _handle is None else _handle
        if _handle is None:
            lib.fbn_network_load_xmlbif(os.fsencode(path), C.byref(h))
        self._h = h
        _register(self)
        n = C.c_int()
        lib.fbn_network_num_nodes(h, C.byref(n))
        self.num_nodes = n.value
        self.dims = np.zeros(self.num_nodes, np.int32)
        lib.fbn_network_dims(h, _p(self.dims))

    @classmethod
    def from_counts(cls, dims, parents, counts, names=None):
        """A network built in memory (fbn_network_create; the reference's Network of DiscreteNodes,
        src/DiscreteNode.cpp:114-147): dims[v] states, parents[v] (the node's own order), counts[v]
        = int [dims[v]][parent configs], configurations over the parents in ascending index order,
        last fastest (map_cond_prob_table_statistics)."""
        n = len(dims)
        d = np.ascontiguousarray(dims, np.int32)
        off = np.zeros(n + 1, np.int32)
        for v in range(n):
            off[v + 1] = off[v] + len(parents[v])
        par = np.ascontiguousarray([q for ps in parents for q in ps] or [0], np.int32)
        cnt = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int64).reshape(-1) for c in counts]), np.int64)
        nm = None
        if names is not None:
            enc = [os.fsencode(x) for x in names]
            nm = (C.c_char_p * n)(*enc)
        h = C.c_void_p()
        lib.fbn_network_create(n, _p(d), _p(off), _p(par), _p(cnt), C.cast(nm, C.c_void_p) if nm is not None else None,
                               C.byref(h))
        return cls(_handle=h)

    @classmethod
    def from_cpts(cls, dims, parents, cpts, names=None):
        """A network that holds probabilities (fbn_network_create_cpt): as from_counts with cpts[v] = fp64
        [dims[v]][parent configs]; every entry finite and > 0, every column summing to 1 within 1e-9."""
        n = len(dims)
        d = np.ascontiguousarray(dims, np.int32)
        off = np.zeros(n + 1, np.int32)
        for v in range(n):
            off[v + 1] = off[v] + len(parents[v])
        par = np.ascontiguousarray([q for ps in parents for q in ps] or [0], np.int32)
        tab = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float64).reshape(-1) for c in cpts]), np.float64)
        nm = None
        if names is not None:
            enc = [os.fsencode(x) for x in names]
            nm = (C.c_char_p * n)(*enc)
        h = C.c_void_p()
        lib.fbn_network_create_cpt(n, _p(d), _p(off), _p(par), _p(tab),
                                   C.cast(nm, C.c_void_p) if nm is not None else None, C.byref(h))
        return cls(_handle=h)

    def node_probs(self, v):
        """(parents ascending, probabilities fp64 [dims[v]][parent configs]) of node v: a probability
        network's entries, or a count network's (count + 1) / (total + dims[v])."""
        npar, n = C.c_int(), C.c_int64()
        lib.fbn_network_node_probs(self._h, int(v), None, None, C.byref(npar), C.byref(n))
        par = np.zeros(max(1, npar.value), np.int32)
        pr = np.zeros(max(1, n.value), np.float64)
        lib.fbn_network_node_probs(self._h, int(v), _p(par), _p(pr), C.byref(npar), C.byref(n))
        return par[:npar.value], pr[:n.value].reshape(int(self.dims[v]), -1)

    def node_counts(self, v):
        """(parents ascending, counts [dims[v]][parent configs]) of node v."""
        npar, ncnt = C.c_int(), C.c_int64()
        lib.fbn_network_node_counts(self._h, int(v), None, None, C.byref(npar), C.byref(ncnt))
        par = np.zeros(max(1, npar.value), np.int32)
        cnt = np.zeros(max(1, ncnt.value), np.int64)
        lib.fbn_network_node_counts(self._h, int(v), _p(par), _p(cnt), C.byref(npar), C.byref(ncnt))
        return par[:npar.value], cnt[:ncnt.value].reshape(int(self.dims[v]), -1)

    def name(self, i):
        buf = C.create_string_buffer(256)
        lib.fbn_network_name(self._h, i, buf, 256)
        return buf.value.decode()

    def forward_sample(self, n, seed):
        """n complete cases, uint8 [V][n] (fbn_synth_forward_sample; = synth.forward_sample)."""
        cols = np.empty((self.num_nodes, n), np.uint8)
        lib.fbn_synth_forward_sample(self._h, int(n), int(seed), _p(cols))
        return cols

    def evidence_cases(self, n, k, seed, query=0):
        """n evidence cases observing k variables each, int8 [n][V] (fbn_synth_evidence; =
        synth.evidence_cases)."""
        ev = np.empty((n, self.num_nodes), np.int8)
        lib.fbn_synth_evidence(self._h, int(n), int(k), int(seed), int(query), _p(ev))
        return ev



def write_csv(path, columns, network=None):
    """CSV of a column store (header + "s<code>" values), the reference's LoadCSVData input."""
    cols = np.ascontiguousarray(columns, np.uint8)
    lib.fbn_write_csv(os.fsencode(path), _p(cols), cols.shape[0], cols.shape[1], network._h if network else None)


def write_libsvm(path, evidence, labels=None):
    """LIBSVM test set of evidence rows (label + observed v:x), the reference's
    LoadLIBSVMDataKnownNetwork input."""
    ev = np.ascontiguousarray(evidence, np.int8)
    lab = None if labels is None else np.ascontiguousarray(labels, np.int32)
    lib.fbn_write_libsvm(os.fsencode(path), _p(ev), ev.shape[0], ev.shape[1], None if lab is None else _p(lab))


def kernel_options():
    """Compile options of the plan-specialized JT kernel (list of str)."""
    buf = C.create_string_buffer(1024)
    lib.fbn_jt_kernel_options(buf, 1024)
    return [x for x in buf.value.decode().split("\n") if x]


def load_libsvm(path, num_nodes):
    """Dataset::LoadLIBSVMDataKnownNetwork + Inference evidence extraction -> (evidence, labels)."""
    n = C.c_int64()
    lib.fbn_evidence_load_libsvm(os.fsencode(path), num_nodes, None, None, 0, C.byref(n))
    ev = np.zeros((n.value, num_nodes), np.int8)
    lab = np.zeros(n.value, np.int32)
    lib.fbn_evidence_load_libsvm(os.fsencode(path), num_nodes, _p(ev), _p(lab), n.value, C.byref(n))
    return ev, lab


class Dataset:
    """CSV training set with first-appearance value coding (Dataset::LoadCSVData)."""

    def __init__(self, path=None, columns=None, dims=None):
        if path is not None:
            h = C.c_void_p()
            lib.fbn_dataset_load_csv(os.fsencode(path), C.byref(h))
            nv, ns = C.c_int(), C.c_int64()
            lib.fbn_dataset_shape(h, C.byref(nv), C.byref(ns))
            self.dims = np.zeros(nv.value, np.int32)
            self.columns = np.zeros((nv.value, ns.value), np.uint8)
            lib.fbn_dataset_dims(h, _p(self.dims))
            lib.fbn_dataset_columns(h, _p(self.columns))
            self.names = []
            buf = C.create_string_buffer(256)
            for v in range(nv.value):
                lib.fbn_dataset_var_name(h, v, buf, 256)
                self.names.append(buf.value.decode())
            lib.fbn_dataset_destroy(h)
        else:
            self.columns = np.ascontiguousarray(columns, dtype=np.uint8)
            self.dims = np.ascontiguousarray(dims, dtype=np.int32)
            self.names = [str(i) for i in range(self.columns.shape[0])]

    @property
    def num_vars(self):
        return self.columns.shape[0]

    @property
    def num_instance(self):
        return self.columns.shape[1]


class JunctionTree(_Handle):
    """Batched JT inference on one device (JunctionTree ctor + PredictUseJTInfer over all cases)."""

    _destroy = "fbn_jt_plan_destroy"
    _create = "fbn_jt_plan_create"

    def __init__(self, network, device=0):
        self.network = network
        h = C.c_void_p()
        getattr(lib, self._create)(network._h, device, C.byref(h))
        self._h = h
        _register(self)
        self.output_layout = 0
        info = _PlanInfo()
        lib.fbn_jt_plan_info_get(h, C.byref(info))
        self.info = {k: getattr(info, k) for k, _ in _PlanInfo._fields_}

    def tile_program(self):
        """The tiled kernel's program (variant 5): (passes [n][32] int32, tab int32, initv fp64,
        geometry dict) -- for host-side checks of its tables (tests/tile_emulator.py)."""
        g = np.zeros(8, np.int64)
        lib.fbn_jt_tile_program(self._h, None, None, None, _p(g))
        passes = np.zeros((int(g[0]), 33), np.int32)
        tab = np.zeros(max(int(g[1]), 1), np.int32)
        iv = np.zeros(max(int(g[2]), 1), np.float64)
        lib.fbn_jt_tile_program(self._h, _p(passes), _p(tab), _p(iv), _p(g))
        keys = ["n_passes", "n_tab", "n_init", "scr_row", "red_row", "store_rows", "cases_per_wave", "slots"]
        return passes, tab, iv, dict(zip(keys, (int(x) for x in g)))

    def dump_plan(self, plan_path, init_path):
        lib.fbn_jt_plan_dump(self._h, os.fsencode(plan_path), os.fsencode(init_path))

    def stream_schedule(self):
        """Streamed-kernel schedule: (order, sched) -- see fbn_jt_stream_schedule."""
        no, ns = C.c_int64(), C.c_int64()
        lib.fbn_jt_stream_schedule(self._h, None, 0, None, 0, C.byref(no), C.byref(ns))
        order = np.zeros(no.value, np.int32)
        sched = np.zeros(ns.value, np.int32)
        lib.fbn_jt_stream_schedule(self._h, _p(order), no.value, _p(sched), ns.value, None, None)
        return order, sched

    def set_waves_per_cu(self, w):
        lib.fbn_jt_set_waves_per_cu(self._h, w)

    def op_cycles(self, enable, read=True):
        """Diagnostic per-op-type cycles of the last run (LDS variant)."""
        buf = np.zeros(10, np.uint64)
        lib.fbn_jt_debug_op_cycles(self._h, int(enable), _p(buf) if read else None)
        names = ["INIT", "MUL", "SEPCOL", "STORE", "LOAD", "DMUL", "SEPDIS", "MARG", "EVZERO", "-"]
        return dict(zip(names, buf.tolist()))

    def kernel_source(self):
        """Source of the plan-specialized kernel (variant 3)."""
        n = C.c_int64()
        lib.fbn_jt_kernel_source(self._h, None, 0, C.byref(n))
        buf = C.create_string_buffer(n.value)
        lib.fbn_jt_kernel_source(self._h, buf, n.value, C.byref(n))
        return buf.value.decode()

    def kernel_cache_path(self):
        buf = C.create_string_buffer(4096)
        lib.fbn_jt_kernel_cache_path(self._h, buf, 4096)
        return buf.value.decode()

    def debug_force_fixup(self, enable):
        lib.fbn_jt_debug_force_fixup(self._h, int(enable))

    def debug_flagged_blocks(self):
        """64-case blocks the last run flagged for the exact fixup (variants 3-5)."""
        n = C.c_int64()
        lib.fbn_jt_debug_flagged_blocks(self._h, C.byref(n))
        return n.value

    def set_exact(self, exact):
        """Arithmetic order of the specialized / streamed kernels: True = the reference's
        (bit-identical), False = fast (normalizations that cancel left out; labels equal, marginals
        within 1e-12), None = auto (fast)."""
        lib.fbn_jt_set_exact(self._h, -1 if exact is None else int(bool(exact)))

    def build_kernel(self):
        """Compile the plan-specialized kernel into the on-disk cache (no GPU needed)."""
        lib.fbn_jt_kernel_build(self._h)
        return self.kernel_cache_path()

    def refresh_info(self):
        info = _PlanInfo()
        lib.fbn_jt_plan_info_get(self._h, C.byref(info))
        self.info = {k: getattr(info, k) for k, _ in _PlanInfo._fields_}
        if self.info["specialized_eligible"]:
            # where the specialized kernel of the current order / layout keeps its message rows
            rows = np.zeros(8, np.int64)
            lib.fbn_jt_kernel_placement(self._h, _p(rows))
            names = ("global_collect", "global_distribute", "lds_collect", "lds_distribute", "reg_collect",
                     "reg_distribute", "workspace", "lds_pool")
            self.info.update({"place_rows_" + k: int(v) for k, v in zip(names, rows)})
        return self.info

    def set_variant(self, v):
        """-1 auto, 0 = clique-in-LDS interpreter, 1 = global-workspace interpreter,
        2 = LDS interpreter with IEEE division, 3 = plan-specialized kernel,
        4 = streamed (virtual-table) kernel for large trees, 5 = per-case evidence-reduced
        kernel for large trees (fast arithmetic order)."""
        lib.fbn_jt_set_variant(self._h, v)

    def infer(self, evidence, marginals=True):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (labels, marginals or None)."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        labels = np.zeros(n, np.int32)
        marg = np.zeros((n, self.info["sum_dom"]), np.float64) if marginals else None
        lib.fbn_jt_run(self._h, _p(ev), n, _p(labels), _p(marg), None)
        return labels, marg

    def run_device(self, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr, stream_ptr=None):
        """Device-resident run (asynchronous on the stream unless the evidence check is on)."""
        lib.fbn_jt_run_device(self._h, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr, stream_ptr)

    def validate_device(self, d_evidence_ptr, ncases, stream_ptr=None):
        """Device-side evidence range check of a device buffer; raises FastBNError if a code is out
        of its node's domain."""
        lib.fbn_jt_evidence_validate(self._h, d_evidence_ptr, ncases, stream_ptr)

    def set_kernel_timing(self, enable):
        """fbn_jt_set_kernel_timing: enable = False records no timing events per run (last_kernel_ms
        then raises); for callers that time with their own events."""
        lib.fbn_jt_set_kernel_timing(self._h, int(bool(enable)))

    def set_evidence_check(self, enable):
        """run_device's per-call evidence check (default on); off = fully asynchronous runs of a
        buffer the caller validated (validate_device)."""
        lib.fbn_jt_set_evidence_check(self._h, int(bool(enable)))

    def set_output_layout(self, layout):
        """fbn_jt_set_output_layout: run_device's marginals 0 = case-major [ncases][sum_dom]
        (default), 1 = variable-major [sum_dom][ncases] (each store writes 64 consecutive cases).
        infer() always returns case-major."""
        lib.fbn_jt_set_output_layout(self._h, int(layout))
        self.output_layout = int(layout)

    def score_terms_device(self, d_marg_ptr, d_golden_ptr, ncases, d_terms_ptr, stream_ptr=None):
        """fbn_jt_score_terms_device: per-case (MSE, HD) terms [ncases][2] fp64 on the device from
        device marginals (the plan's output layout) and a case-major device golden table."""
        lib.fbn_jt_score_terms_device(self._h, d_marg_ptr, d_golden_ptr, ncases, d_terms_ptr, stream_ptr)

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_jt_last_kernel_ms(self._h, C.byref(ms))
        return ms.value

    def score(self, marginals, golden):
        mse, hd = C.c_double(), C.c_double()
        m = np.ascontiguousarray(marginals, np.float64)
        g = np.ascontiguousarray(golden, np.float64)
        lib.fbn_jt_score(self._h, _p(m), _p(g), m.shape[0], C.byref(mse), C.byref(hd))
        return mse.value, hd.value

    def EvaluateAccuracy(self, evidence, ground_truths, golden=None):
        """Accuracy of the query-variable arg-max (+ average MSE/HD vs golden if given)."""
        labels, marg = self.infer(evidence)
        acc = float(np.mean(labels == np.asarray(ground_truths)))
        if golden is None:
            return acc
        mse, hd = self.score(marg, golden)
        return acc, mse / len(labels), hd / len(labels)


class JunctionForest(JunctionTree):
    """JunctionTree for any DAG (fbn_jt_forest_plan_create): where the moral graph is disconnected --
    JunctionTree raises -- one tree per component, none joined to another, so the cost is the sum of
    the trees' and exact inference stays exact.  On a connected network it is JunctionTree's plan.
    components: the moral graph's components as sorted node lists, ordered by their lowest node."""

    _create = "fbn_jt_forest_plan_create"

    def __init__(self, network, device=0):
        super().__init__(network, device)
        comp = np.zeros(self.info["num_nodes"], np.int32)
        n = C.c_int32()
        lib.fbn_jt_plan_components(self._h, _p(comp), C.byref(n))
        self.components = [np.flatnonzero(comp == k).tolist() for k in range(n.value)]


class IndependenceTest(_Handle):
    """G^2 tests on the device (IndependenceTest::IndependenceResult, batched)."""

    _destroy = "fbn_ci_ctx_destroy"

    def __init__(self, dataset, alpha=0.05, device=0):
        self.alpha = alpha
        self.dims = np.ascontiguousarray(dataset.dims, np.int32)
        self.num_samples = int(dataset.num_instance)
        h = C.c_void_p()
        lib.fbn_ci_dataset_upload(_p(dataset.columns), dataset.num_vars, dataset.num_instance,
                                  _p(dataset.dims), device, C.byref(h))
        self._h = h
        _register(self)

    @classmethod
    def from_device(cls, d_cols_ptr, nvars, nsamples, dims, alpha=0.05, device=0):
        """Column store already in `device` memory (uint8 [nvars][nsamples], e.g. a tensor filled by
        an RCCL broadcast): fbn_ci_dataset_from_device."""
        self = cls.__new__(cls)
        self.alpha = alpha
        dims = np.ascontiguousarray(dims, np.int32)
        self.dims = dims
        self.num_samples = int(nsamples)
        h = C.c_void_p()
        lib.fbn_ci_dataset_from_device(C.c_void_p(d_cols_ptr), int(nvars), int(nsamples), _p(dims), device,
                                       C.byref(h))
        self._h = h
        _register(self)
        return self

    def set_kernel_timing(self, enable):
        """HIP-event kernel timing of every CI launch (default on; off saves the events' cost)."""
        lib.fbn_ci_set_kernel_timing(self._h, int(bool(enable)))

    def level(self, d, edges, e_begin, e_end, group_size=1):
        """One skeleton level for edges[e_begin:e_end] of the current skeleton (fbn_pc_level) ->
        (removed[bool], sepsets[list of tuples or None], counted, launched)."""
        ev = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 2))
        n = e_end - e_begin
        rm = np.zeros(max(n, 1), np.uint8)
        sp = np.zeros((max(n, 1), max(d, 1)), np.int32)
        cnt, lau = C.c_int64(), C.c_int64()
        lib.fbn_pc_level(self._h, self.alpha, d, group_size, _p(ev), ev.shape[0], e_begin, e_end, _p(rm), _p(sp),
                         C.byref(cnt), C.byref(lau))
        rm = rm[:n].astype(bool)
        seps = [tuple(int(v) for v in sp[i, :d]) if rm[i] else None for i in range(n)]
        return rm, seps, cnt.value, lau.value

    def run(self, items, d):
        items = np.ascontiguousarray(items, dtype=np.int32).reshape(-1, 2 + d)
        n = items.shape[0]
        g2 = np.zeros(n)
        df = np.zeros(n, np.int32)
        p = np.zeros(n)
        ind = np.zeros(n, np.uint8)
        lib.fbn_ci_run(self._h, _p(items), n, d, self.alpha, _p(g2), _p(df), _p(p), _p(ind), None)
        return g2, df, p, ind.astype(bool)

    def IndependenceResult(self, x, y, z=()):
        g2, df, p, ind = self.run(np.array([[x, y, *z]], np.int32), len(z))
        return {"g2": g2[0], "df": int(df[0]), "p_value": p[0], "is_independent": bool(ind[0])}

    def production_counts(self, items, d, cap=None):
        """Counts of the tests `items` [n][2+d] through the kernels a PC run uses at level d
        (fbn_ci_debug_counts: level-0 Gram + pair tables, derived level-1 counting, histogram
        kernel) -> int32 [n][cap] (Counts3D order; cells beyond a test's table are 0)."""
        items = np.ascontiguousarray(items, np.int32).reshape(-1, 2 + d)
        if cap is None:
            dims = np.asarray(self.dims)
            cap = int(np.max(np.prod(dims[items], axis=1))) if len(items) else 1
        out = np.zeros((len(items), cap), np.int32)
        lib.fbn_ci_debug_counts(self._h, _p(items), len(items), d, _p(out), cap)
        return out

    def level0_info(self):
        """The last level-0 all-pairs launch of this context (fbn_ci_level0_info): path (1 popcount
        Gram, 2 MFMA Gram, 3 tiled pairs kernel, 0 none yet), R, Rp, KS, nt, S and the shortest /
        longest split-K slice in stages."""
        out = np.zeros(8, np.int64)
        lib.fbn_ci_level0_info(self._h, _p(out))
        keys = ("path", "R", "Rp", "KS", "nt", "S", "shortest", "longest")
        return {k: int(v) for k, v in zip(keys, out)}

    def level0_range_counts(self, pair0, n):
        """The complete-graph pairs [pair0, pair0 + n) as one batch of the PC driver's level-0 chunk
        loop, the level-0 Gram poisoned first (fbn_ci_debug_level0_range) -> int32 [n][16]."""
        out = np.zeros((n, 16), np.int32)
        lib.fbn_ci_debug_level0_range(self._h, int(pair0), int(n), _p(out))
        return out

    def counts(self, x, y, z=()):
        zz = np.array(z, np.int32)
        cells = C.c_int64()
        lib.fbn_ci_counts(self._h, x, y, _p(zz) if len(z) else None, len(z), None, 0, C.byref(cells))
        out = np.zeros(cells.value, np.int32)
        lib.fbn_ci_counts(self._h, x, y, _p(zz) if len(z) else None, len(z), _p(out), cells.value,
                          C.byref(cells))
        return out

    def decision_margin(self, reset=False):
        """(min |p - alpha|, #tests with |p - alpha| < 1e-9) over the tests run since the last reset."""
        m, near = C.c_double(), C.c_int64()
        lib.fbn_ci_decision_margin(self._h, C.byref(m), C.byref(near), int(bool(reset)))
        return m.value, near.value

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_ci_last_kernel_ms(self._h, C.byref(ms))
        return ms.value



class PCResult(_Handle):
    """A PC-stable result handle: skeleton, sepsets, orientation, SHD (fbn_pc_*)."""

    _destroy = "fbn_pc_result_destroy"

    def __init__(self, handle):
        self._h = handle
        _register(self)
        self._edges = self._sepset = self._oriented = None
        m, near = C.c_double(), C.c_int64()
        lib.fbn_pc_decision_margin(handle, C.byref(m), C.byref(near))
        # p-values are parity-unpinned; decisions this close to alpha are flagged
        self.min_margin, self.near_alpha = m.value, near.value
        nl = C.c_int()
        lib.fbn_pc_num_levels(handle, C.byref(nl))
        self.tests_per_level = np.zeros(nl.value, np.int64)
        self.launched_per_level = np.zeros(nl.value, np.int64)
        if nl.value:
            lib.fbn_pc_level_tests(handle, _p(self.tests_per_level))
            lib.fbn_pc_level_launched(handle, _p(self.launched_per_level))
        self.num_ci_test = int(self.tests_per_level.sum())
        tot, ker = C.c_double(), C.c_double()
        lib.fbn_pc_timing(handle, C.byref(tot), C.byref(ker))
        self.total_s, self.kernel_s = tot.value, ker.value
        path = C.c_int()
        lib.fbn_pc_path(handle, C.byref(path))
        # 0 host-driven levels, 1 device-resident search, 2 device-resident search fell back to the host
        self.path = path.value
        nb = C.c_int64()
        lib.fbn_pc_device_bytes(handle, C.byref(nb))
        self.device_bytes = nb.value

    @classmethod
    def with_levels(cls, handle):
        return cls(handle)

    # skeleton / sepsets / orientation are converted to Python objects on first access (a
    # 1000-variable run has ~500k sepsets: the conversion costs far more than the search)
    @property
    def edges(self):
        if self._edges is None:
            ne = C.c_int()
            lib.fbn_pc_num_edges(self._h, C.byref(ne))
            e = np.zeros((max(ne.value, 1), 2), np.int32)
            if ne.value:
                lib.fbn_pc_edges(self._h, _p(e))
            self._edges = [tuple(map(int, x)) for x in e[:ne.value]]
        return self._edges

    @property
    def sepset(self):
        if self._sepset is None:
            ln = C.c_int64()
            lib.fbn_pc_sepsets(self._h, None, 0, C.byref(ln))
            buf = np.zeros(max(ln.value, 1), np.int32)
            lib.fbn_pc_sepsets(self._h, _p(buf), ln.value, C.byref(ln))
            sep, k, b = {}, 0, buf.tolist()
            while k < ln.value:
                x, y, m = b[k], b[k + 1], b[k + 2]
                sep[(x, y)] = tuple(b[k + 3:k + 3 + m])
                k += 3 + m
            self._sepset = sep
        return self._sepset

    @property
    def oriented(self):
        """(from, to, 1) arcs and (min, max, 0) undirected edges, in vec_edges order."""
        if self._oriented is None:
            no = C.c_int()
            lib.fbn_pc_num_oriented_edges(self._h, C.byref(no))
            t = np.zeros((max(no.value, 1), 3), np.int32)
            if no.value:
                lib.fbn_pc_oriented_edges(self._h, _p(t))
            self._oriented = [tuple(map(int, x)) for x in t[:no.value]]
        return self._oriented

    def GetSHD(self, bif_path):
        """BNSLComparison(ref_net, network).GetSHD() with ref_net loaded from a BIF file."""
        shd = C.c_int()
        lib.fbn_pc_shd_bif(self._h, os.fsencode(bif_path), C.byref(shd))
        return shd.value



def shd_bif(bif_path, nvars, oriented):
    """SHD of a learned graph [(from, to, 1) | (a, b, 0)] vs the CPDAG of a BIF DAG."""
    t = np.ascontiguousarray(np.asarray(oriented if oriented else [(0, 0, 0)], np.int32).reshape(-1, 3))
    shd = C.c_int()
    lib.fbn_shd_bif(os.fsencode(bif_path), int(nvars), _p(t), len(oriented), C.byref(shd))
    return shd.value


def orient_skeleton(nvars, edges, sepset):
    """Host-only orientation of a given skeleton (PCStable steps 2-3) -> PCResult."""
    pairs = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 2))
    rec = []
    for (x, y), z in sorted(sepset.items()):
        rec += [x, y, len(z)] + list(z)
    rec = np.ascontiguousarray(np.asarray(rec if rec else [0], np.int32))
    r = C.c_void_p()
    lib.fbn_pc_orient_skeleton(int(nvars), _p(pairs), int(pairs.shape[0]), _p(rec), len(rec) if sepset else 0,
                               C.byref(r))
    return PCResult(r)


class PCStable:
    """PC-stable (PCStable(net, alpha, depth).StructLearnCompData): device skeleton + host orientation."""

    def __init__(self, alpha=0.05, depth=1000, device=0):
        self.alpha, self.depth, self.device = alpha, depth, device
        self.result = None
        self.ci = None

    def StructLearnCompData(self, dataset, group_size=1, num_threads=1, print_struct=False, verbose=False):
        """`dataset`: a Dataset (uploaded for this call) or an IndependenceTest whose column store is
        already resident on the device (reused across calls)."""
        ci = dataset if isinstance(dataset, IndependenceTest) else IndependenceTest(dataset, self.alpha, self.device)
        self.ci = ci  # the context of the run: ParameterLearning(pc.ci) learns from the same upload
        r = C.c_void_p()
        lib.fbn_pc_stable(ci._h, self.alpha, self.depth, group_size, C.byref(r))
        self.result = res = PCResult(r)
        self.tests_per_level, self.launched_per_level = res.tests_per_level, res.launched_per_level
        self.total_s, self.kernel_s, self.device_bytes = res.total_s, res.kernel_s, res.device_bytes
        self.num_ci_test = res.num_ci_test
        self.min_margin, self.near_alpha = self.result.min_margin, self.result.near_alpha
        return self

    edges = property(lambda self: self.result.edges)
    sepset = property(lambda self: self.result.sepset)
    oriented = property(lambda self: self.result.oriented)
    path = property(lambda self: self.result.path)  # 0 host levels, 1 device-resident, 2 fell back, 3 host levels after the device level 0 -> 1 hand-off

    def GetSHD(self, bif_path):
        return self.result.GetSHD(bif_path)


def _csr_parents(parents, nvars):
    """List of parent lists -> (parent_off int32 [nvars+1], parents int32) for the C-ABI."""
    if len(parents) != nvars:
        raise FastBNError(f"{len(parents)} parent lists for {nvars} variables")
    off = np.zeros(nvars + 1, np.int32)
    for v in range(nvars):
        off[v + 1] = off[v] + len(parents[v])
    par = np.ascontiguousarray([int(q) for ps in parents for q in ps] or [0], np.int32)
    return off, par


def family_sizes(dims, parents):
    """fbn_param_family_sizes: (family_off int64 [n+1], total cells) of the tables counts[v] =
    [dims[v]][parent configurations]; raises FastBNError for a bad parent list (code -1) or a graph
    past the cell cap (code -6).  Host only."""
    d = np.ascontiguousarray(dims, np.int32)
    off, par = _csr_parents(parents, len(d))
    foff = np.zeros(len(d) + 1, np.int64)
    total = C.c_int64()
    lib.fbn_param_family_sizes(len(d), _p(d), _p(off), _p(par), _p(foff), C.byref(total))
    return foff, total.value


def pdag_to_dag(nvars, oriented):
    """fbn_pdag_to_dag: a consistent DAG extension (Dor & Tarsi) of a PDAG given as PCResult.oriented
    gives it -- (from, to, 1) arcs and (a, b, 0) undirected edges -- as a list of ascending parent
    lists.  Deterministic; raises FastBNError if no extension exists.  Host only."""
    n = len(oriented)
    t = np.ascontiguousarray(np.asarray(oriented if n else [(0, 0, 0)], np.int32).reshape(-1, 3))
    off = np.zeros(int(nvars) + 1, np.int32)
    par = np.zeros(max(n, 1), np.int32)
    lib.fbn_pdag_to_dag(int(nvars), _p(t), n, _p(off), _p(par))
    return [[int(q) for q in par[off[v]:off[v + 1]]] for v in range(int(nvars))]


class ParameterLearning:
    """Maximum-likelihood counts of a known structure from complete data on the device
    (ParameterLearning::LearnParamsKnowStructCompData).  `source`: a Dataset (uploaded here) or an
    IndependenceTest, whose context -- and column store -- is shared, so PC-stable and learning use
    one upload (PCStable.ci after a run)."""

    def __init__(self, source, device=0):
        self.ci = source if isinstance(source, IndependenceTest) else IndependenceTest(source, device=device)
        self.dims = np.ascontiguousarray(self.ci.dims, np.int32)

    def counts(self, parents):
        """Family counts of every node: a list of int64 [dims[v]][parent configurations] arrays
        (configurations over the parents in ascending index order, last fastest), the shape
        Network.node_counts returns."""
        n = len(self.dims)
        off, par = _csr_parents(parents, n)
        total = C.c_int64()
        lib.fbn_param_counts(self.ci._h, _p(off), _p(par), None, 0, C.byref(total))
        buf = np.zeros(max(total.value, 1), np.int64)
        lib.fbn_param_counts(self.ci._h, _p(off), _p(par), _p(buf), total.value, C.byref(total))
        out, o = [], 0
        for v in range(n):
            cells = int(self.dims[v]) * int(np.prod(self.dims[list(parents[v])], dtype=np.int64))
            out.append(buf[o:o + cells].reshape(int(self.dims[v]), -1))
            o += cells
        return out

    def LearnParamsKnowStructCompData(self, parents, names=None):
        """The learned Network (fbn_param_learn): parents[v] in the node's own order."""
        n = len(self.dims)
        off, par = _csr_parents(parents, n)
        nm = None
        if names is not None:
            enc = [os.fsencode(x) for x in names]
            nm = (C.c_char_p * n)(*enc)
        h = C.c_void_p()
        lib.fbn_param_learn(self.ci._h, _p(off), _p(par), C.cast(nm, C.c_void_p) if nm is not None else None,
                            C.byref(h))
        return Network(_handle=h)

    def set_tuning(self, samples_per_slice=0, lds_cells_max=0):
        """fbn_param_set_tuning: samples per (family, slice) work item and the largest table counted
        in LDS; 0 = default."""
        lib.fbn_param_set_tuning(self.ci._h, int(samples_per_slice), int(lds_cells_max))

    def last_kernel_ms(self):
        return self.ci.last_kernel_ms()


def hc_penalty(score, nsamples):
    """fbn_hc_penalty: the penalty of a named score ("bic", "aic", "loglik"), or a number as it is."""
    if isinstance(score, str):
        p = C.c_double()
        lib.fbn_hc_penalty(score.encode(), int(nsamples), C.byref(p))
        return p.value
    return float(score)


def hc_table_bytes(nsamples):
    """fbn_hc_table_bytes: bytes of the n ln n table of `nsamples` samples (code -6 past 2^24).  Host only."""
    b = C.c_int64()
    lib.fbn_hc_table_bytes(int(nsamples), C.byref(b))
    return b.value


def _csr_families(families):
    """[(child, parents...)] -> (fam_off int64 [n+1], fam_cols int32) for the C-ABI."""
    off = np.zeros(len(families) + 1, np.int64)
    for f, fam in enumerate(families):
        off[f + 1] = off[f] + len(fam)
    cols = np.ascontiguousarray([int(v) for fam in families for v in fam] or [0], np.int32)
    return off, cols


def family_scores(source, families, penalty=0.0):
    """fbn_score_families: (loglik, score) float64 arrays of the families [(child, parent, ...), ...] from
    the column store resident in `source` (an IndependenceTest: on the device), or, for a Dataset,
    fbn_score_families_host: the host twin, bit-identical, no device."""
    off, cols = _csr_families(families)
    n = len(families)
    ll, sc = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    if isinstance(source, IndependenceTest):
        lib.fbn_score_families(source._h, float(penalty), n, _p(off), _p(cols), _p(ll), _p(sc))
    else:
        lib.fbn_score_families_host(source.num_vars, _p(source.dims), _p(source.columns), source.num_instance,
                                    float(penalty), n, _p(off), _p(cols), _p(ll), _p(sc))
    return ll[:n], sc[:n]


class _HcOptions(C.Structure):
    _fields_ = [("penalty", C.c_double), ("max_parents", C.c_int32), ("max_iter", C.c_int32),
                ("max_family_cells", C.c_int64), ("allowed", C.c_void_p), ("allowed_len", C.c_int64),
                ("start_off", C.c_void_p), ("start_parents", C.c_void_p)]


class _HcInfo(C.Structure):
    _fields_ = [("nvars", C.c_int32), ("narcs", C.c_int32), ("iterations", C.c_int32), ("pad", C.c_int32),
                ("families_scored", C.c_int64), ("batches", C.c_int64), ("score", C.c_double), ("loglik", C.c_double),
                ("kernel_ms", C.c_double), ("first_sweep_kernel_ms", C.c_double), ("first_sweep_wall_ms", C.c_double),
                ("score_wall_ms", C.c_double), ("wall_ms", C.c_double)]


class HillClimbing:
    """Score-based structure learning: greedy hill climbing over arc additions, deletions and reversals
    (fbn_hc_run; no reference counterpart).  score: "bic" | "aic" | "loglik" or an explicit non-negative
    penalty per free parameter.  allowed: [n][n] mask, allowed[x][y] lets the search add x -> y; start: a DAG
    as parent lists.  learn(source): a Dataset (uploaded here), or an IndependenceTest, whose context is
    shared (`.ci`, as PCStable.ci: ParameterLearning(hc.ci) learns from the same upload); host=True runs
    the host twin (fbn_hc_run_host) on a Dataset, without a device.  Results: .parents (ascending parent
    lists), .score, .loglik, .node_scores, .trace [(type, from, to, delta)] (type 0 add, 1 delete,
    2 reverse), .iterations, .families_scored, .kernel_ms, .info."""

    OPS = ("add", "delete", "reverse")

    def __init__(self, score="bic", max_parents=None, max_family_cells=0, max_iter=None, allowed=None, start=None,
                 device=0):
        self.score_name, self.device = score, device
        self.max_parents, self.max_family_cells, self.max_iter = max_parents, max_family_cells, max_iter
        self.allowed, self.start = allowed, start
        self.ci = None

    def _options(self, nvars, nsamples):
        o = _HcOptions()
        o.penalty = hc_penalty(self.score_name, nsamples)
        o.max_parents = -1 if self.max_parents is None else int(self.max_parents)
        o.max_iter = -1 if self.max_iter is None else int(self.max_iter)
        o.max_family_cells = int(self.max_family_cells)
        keep = []
        if self.allowed is not None:
            a = np.ascontiguousarray(np.asarray(self.allowed) != 0, np.uint8)
            keep.append(a)
            o.allowed, o.allowed_len = a.ctypes.data, a.size
        if self.start is not None:
            off, par = _csr_parents(self.start, nvars)
            keep += [off, par]
            o.start_off, o.start_parents = off.ctypes.data, par.ctypes.data
        return o, keep

    def learn(self, source, host=False):
        r = C.c_void_p()
        if host:
            o, keep = self._options(source.num_vars, source.num_instance)
            lib.fbn_hc_run_host(source.num_vars, _p(source.dims), _p(source.columns), source.num_instance, C.byref(o),
                                C.byref(r))
        else:
            ci = source if isinstance(source, IndependenceTest) else IndependenceTest(source, device=self.device)
            self.ci = ci
            o, keep = self._options(len(ci.dims), ci.num_samples)
            lib.fbn_hc_run(ci._h, C.byref(o), C.byref(r))
        del keep
        try:
            info = _HcInfo()
            lib.fbn_hc_result_info(r, C.byref(info))
            n, it = info.nvars, info.iterations
            off, par = np.zeros(n + 1, np.int32), np.zeros(max(info.narcs, 1), np.int32)
            lib.fbn_hc_result_parents(r, _p(off), _p(par))
            ns_, nl = np.zeros(n), np.zeros(n)
            lib.fbn_hc_result_node_scores(r, _p(ns_), _p(nl))
            ops, delta = np.zeros((max(it, 1), 3), np.int32), np.zeros(max(it, 1))
            lib.fbn_hc_result_trace(r, _p(ops), _p(delta))
        finally:
            lib.fbn_hc_result_destroy(r)
        self.parents = [[int(q) for q in par[off[v]:off[v + 1]]] for v in range(n)]
        self.score, self.loglik = info.score, info.loglik
        self.node_scores, self.node_logliks = ns_, nl
        self.trace = [(int(ops[k, 0]), int(ops[k, 1]), int(ops[k, 2]), float(delta[k])) for k in range(it)]
        self.iterations, self.families_scored, self.kernel_ms = it, info.families_scored, info.kernel_ms
        self.info = {k: getattr(info, k) for k, _ in _HcInfo._fields_ if k != "pad"}
        return self

    @property
    def oriented(self):
        """The learned arcs as (from, to, 1) triples, the form shd_bif and pdag_to_dag take."""
        return [(q, v, 1) for v, ps in enumerate(self.parents) for q in ps]

    @staticmethod
    def set_tuning(ci, chunk_cells_max=0):
        """fbn_hc_set_tuning on a context: the most table cells per chunk of a batch; 0 = default."""
        lib.fbn_hc_set_tuning(ci._h, int(chunk_cells_max))


def score_marginals(network, marginals, golden):
    """fbn_score_marginals: (mse_sum, hd_sum) of marginals [n][sum_dom] against a golden table, as
    JunctionTree.score computes them, from the network alone (no plan)."""
    m = np.ascontiguousarray(marginals, np.float64)
    g = np.ascontiguousarray(golden, np.float64)
    mse, hd = C.c_double(), C.c_double()
    lib.fbn_score_marginals(network._h, _p(m), _p(g), m.shape[0], C.byref(mse), C.byref(hd))
    return mse.value, hd.value


class _CaseInference:
    """What the approximate case-inference classes share: the buffers of infer and debug_samples, the
    eps argument and EvaluateAccuracy.  The class sets self.network and self.sum_dom and defines infer."""

    def _outputs(self, evidence, marginals, k):
        """(evidence int8, ncases, labels, marginals or None, stats [ncases][k]) of one infer call."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        labels = np.zeros(n, np.int32)
        marg = np.zeros((n, self.sum_dom), np.float64) if marginals else None
        return ev, n, labels, marg, np.zeros((n, k), np.float64)

    def _debug_outputs(self, evidence, draws):
        """(evidence int8, ncases, values, mantissas, exponents) for `draws` samples per case."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        tot = n * draws
        return (ev, n, np.zeros((self.network.num_nodes, tot), np.uint8), np.zeros(tot, np.float64),
                np.zeros(tot, np.int32))

    @staticmethod
    def _eps_arg(eps):
        """The C entries' eps: None -> -1.0 (they read a negative eps as "the defaults")."""
        if eps is None:
            return -1.0
        if float(eps) < 0.0:
            err = FastBNError(f"eps {eps!r}: in [0, 1), or None for the defaults")
            err.code = -1  # FBN_ERR_ARG
            raise err
        return float(eps)

    def EvaluateAccuracy(self, evidence, ground_truths, golden=None):
        """Accuracy of the query-variable arg-max (+ average MSE/HD vs golden if given)."""
        labels, marg = self.infer(evidence)
        acc = float(np.mean(labels == np.asarray(ground_truths)))
        if golden is None:
            return acc
        mse, hd = score_marginals(self.network, marg, golden)
        return acc, mse / len(labels), hd / len(labels)


class Sampler(_Handle):
    """The sampling engine of one network on one device (fbn_sampler).  device < 0: the host path,
    the same algorithm on CPU threads (bit-identical results)."""

    _destroy = "fbn_sampler_destroy"

    def __init__(self, network, device=0):
        self.network = network
        h = C.c_void_p()
        lib.fbn_sampler_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def forward_sample(self, n, seed):
        """n complete cases, uint8 [V][n]; = Network.forward_sample(n, seed) = synth.forward_sample."""
        cols = np.empty((self.network.num_nodes, int(n)), np.uint8)
        lib.fbn_sample_forward(self._h, int(n), int(seed), _p(cols))
        return cols

    def forward_sample_device(self, d_cols_ptr, n, seed, stream_ptr=None):
        """The same into a device buffer uint8 [V][n] (e.g. IndependenceTest.from_device's input);
        asynchronous on the stream."""
        lib.fbn_sample_forward_device(self._h, int(n), int(seed), C.c_void_p(d_cols_ptr), stream_ptr)

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_sampler_last_kernel_ms(self._h, C.byref(ms))
        return ms.value


class LikelihoodWeighting(_CaseInference, Sampler):
    """Sampling inference, mirroring JunctionTree: likelihood weighting (method="lw", the reference's
    -a 5) or probabilistic logic sampling ("pls", -a 4) with num_samples samples per case (-q).
    Works on any DAG, a disconnected learned network included."""

    _METHODS = {"lw": 0, "pls": 1}

    def __init__(self, network, num_samples=10000, seed=0, device=0, method="lw"):
        if method not in self._METHODS:
            raise FastBNError(f"method {method!r}: 'lw' or 'pls'")
        super().__init__(network, device)
        self.num_samples, self.seed, self.method = int(num_samples), int(seed), self._METHODS[method]
        self.sum_dom = int(np.sum(network.dims))
        self.stats = None

    def infer(self, evidence, marginals=True, case_offset=0):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (labels, marginals or None);
        self.stats = (log_evidence, ess) per case.  case_offset: the global index of the first case
        (a batch split over calls gives the bits of the whole batch)."""
        ev, n, labels, marg, st = self._outputs(evidence, marginals, 2)
        lib.fbn_lw_run(self._h, self.method, _p(ev), n, self.num_samples, self.seed, int(case_offset), _p(labels),
                       _p(marg), _p(st))
        self.stats = (st[:, 0].copy(), st[:, 1].copy())
        return labels, marg

    def run_device(self, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr, d_stats_ptr=None, case_offset=0,
                   stream_ptr=None):
        """Device-resident run (asynchronous on the stream after the evidence check)."""
        lib.fbn_lw_run_device(self._h, self.method, C.c_void_p(d_evidence_ptr), int(ncases), self.num_samples,
                              self.seed, int(case_offset), C.c_void_p(d_labels_ptr),
                              C.c_void_p(d_marg_ptr) if d_marg_ptr else None,
                              C.c_void_p(d_stats_ptr) if d_stats_ptr else None, stream_ptr)

    def debug_samples(self, evidence, case_offset=0):
        """The samples behind infer(evidence): (values uint8 [V][ncases * S], mantissas fp64,
        exponents int32 [ncases * S]); sample s of case c at c * S + s."""
        ev, n, vals, m, e = self._debug_outputs(evidence, self.num_samples)
        lib.fbn_lw_debug_samples(self._h, self.method, _p(ev), n, self.num_samples, self.seed, int(case_offset),
                                 _p(vals), _p(m), _p(e))
        return vals, m, e


class LoopyBeliefPropagation(_CaseInference, _Handle):
    """Loopy belief propagation (fbn_lbp; the reference's -a 7 stub, src/main.cpp:136-147), mirroring
    JunctionTree: `iterations` flooding sweeps (the reference's propagation length, -d), stopping
    early once an iteration's residual is <= tol; `damping` in [0, 1) on the factor -> variable
    messages.  Exact on forests / polytrees, an approximation on loopy graphs.  Works on any DAG, a
    disconnected learned network included.  device < 0: the host twin (bit-identical results)."""

    _destroy = "fbn_lbp_destroy"

    def __init__(self, network, iterations=2, tol=0.0, damping=0.0, device=0):
        self.network = network
        self.iterations, self.tol, self.damping = int(iterations), float(tol), float(damping)
        self.sum_dom = int(np.sum(network.dims))
        self.stats = None
        h = C.c_void_p()
        lib.fbn_lbp_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def info(self):
        """dict(edges, msg_doubles, lds_bytes, path): path 0 = messages in LDS, 1 = global workspace."""
        e, m, b, p = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        lib.fbn_lbp_info(self._h, C.byref(e), C.byref(m), C.byref(b), C.byref(p))
        return {"edges": e.value, "msg_doubles": m.value, "lds_bytes": b.value, "path": p.value}

    def infer(self, evidence, marginals=True):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (labels, marginals or None);
        self.stats = (iterations used, last residual) per case."""
        ev, n, labels, marg, st = self._outputs(evidence, marginals, 2)
        lib.fbn_lbp_run(self._h, _p(ev), n, self.iterations, self.tol, self.damping, _p(labels), _p(marg), _p(st))
        self.stats = (st[:, 0].astype(np.int32), st[:, 1].copy())
        return labels, marg

    def run_device(self, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr, d_stats_ptr=None, stream_ptr=None):
        """Device-resident run (asynchronous on the stream after the evidence check)."""
        lib.fbn_lbp_run_device(self._h, C.c_void_p(d_evidence_ptr), int(ncases), self.iterations, self.tol,
                               self.damping, C.c_void_p(d_labels_ptr), C.c_void_p(d_marg_ptr) if d_marg_ptr else None,
                               C.c_void_p(d_stats_ptr) if d_stats_ptr else None, stream_ptr)

    def debug_messages(self, evidence, iterations):
        """Both message arrays [ncases][2][msg_doubles] (factor -> variable, then variable ->
        factor) after exactly `iterations` iterations."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        out = np.zeros((n, 2, self.info()["msg_doubles"]), np.float64)
        lib.fbn_lbp_debug_messages(self._h, _p(ev), n, int(iterations), self.damping, _p(out))
        return out

    def set_tuning(self, lds_bytes_max=0, max_groups=0):
        """fbn_lbp_set_tuning: lds_bytes_max < 0 forces the global message workspace; max_groups caps
        the persistent grid.  0 = default.  Results do not change."""
        lib.fbn_lbp_set_tuning(self._h, int(lds_bytes_max), int(max_groups))

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_lbp_last_kernel_ms(self._h, C.byref(ms))
        return ms.value


class EPISBN(_CaseInference, _Handle):
    """EPIS-BN (fbn_epis; the reference's -a 6 stub, src/main.cpp:123-134), mirroring JunctionTree:
    `iterations` sweeps of loopy belief propagation (tol, damping as LoopyBeliefPropagation), then
    importance sampling with num_samples samples per case (-q) from each CPT row times the lambda
    message LBP left on the variable.  eps: the cutoff in [0, 1), None = the defaults by state count.
    iterations=0 is likelihood weighting's draws.  Unbiased; works on any DAG, a disconnected learned
    network included.  device < 0: the host twin (bit-identical results)."""

    _destroy = "fbn_epis_destroy"

    def __init__(self, network, num_samples=10000, iterations=20, tol=0.0, damping=0.0, eps=None, seed=0, device=0):
        self.network = network
        self.num_samples, self.seed = int(num_samples), int(seed)
        self.iterations, self.tol, self.damping = int(iterations), float(tol), float(damping)
        self.eps = self._eps_arg(eps)
        self.sum_dom = int(np.sum(network.dims))
        self.stats = None
        h = C.c_void_p()
        lib.fbn_epis_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def _run_args(self, n, case_offset):
        return (n, self.num_samples, self.seed, int(case_offset), self.iterations, self.tol, self.damping, self.eps)

    def infer(self, evidence, marginals=True, case_offset=0):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (labels, marginals or None);
        self.stats = (log_evidence, ess, LBP iterations used, LBP residual) per case.  case_offset: the
        global index of the first case (a batch split over calls gives the bits of the whole batch)."""
        ev, n, labels, marg, st = self._outputs(evidence, marginals, 4)
        lib.fbn_epis_run(self._h, _p(ev), *self._run_args(n, case_offset), _p(labels), _p(marg), _p(st))
        self.stats = (st[:, 0].copy(), st[:, 1].copy(), st[:, 2].astype(np.int32), st[:, 3].copy())
        return labels, marg

    def run_device(self, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr=None, d_stats_ptr=None, case_offset=0,
                   stream_ptr=None):
        """Device-resident run (two launches, asynchronous on the stream after the evidence check);
        d_stats [ncases][4]."""
        lib.fbn_epis_run_device(self._h, C.c_void_p(d_evidence_ptr), *self._run_args(int(ncases), case_offset),
                                C.c_void_p(d_labels_ptr), C.c_void_p(d_marg_ptr) if d_marg_ptr else None,
                                C.c_void_p(d_stats_ptr) if d_stats_ptr else None, stream_ptr)

    def debug_samples(self, evidence, case_offset=0):
        """The samples behind infer(evidence): (values uint8 [V][ncases * S], mantissas fp64, exponents
        int32 [ncases * S], lambda rows fp64 [ncases][sum_dom]); sample s of case c at c * S + s."""
        ev, n, vals, m, e = self._debug_outputs(evidence, self.num_samples)
        lam = np.zeros((n, self.sum_dom), np.float64)
        lib.fbn_epis_debug_samples(self._h, _p(ev), *self._run_args(n, case_offset), _p(vals), _p(m), _p(e), _p(lam))
        return vals, m, e, lam

    def set_tuning(self, lds_bytes_max=0):
        """fbn_epis_set_tuning: lds_bytes_max < 0 reads the lambda rows from global memory instead of
        LDS; 0 = default.  Results do not change."""
        lib.fbn_epis_set_tuning(self._h, int(lds_bytes_max))

    def info(self):
        """dict(lds_bytes, path): path 0 = the lambda row in LDS, 1 = in global memory."""
        b, p = C.c_int64(), C.c_int()
        lib.fbn_epis_info(self._h, C.byref(b), C.byref(p))
        return {"lds_bytes": b.value, "path": p.value}

    def last_kernel_ms(self):
        """(LBP kernel ms, sampling kernel ms) of the last run."""
        a, b = C.c_float(), C.c_float()
        lib.fbn_epis_last_kernel_ms(self._h, C.byref(a), C.byref(b))
        return a.value, b.value


class AISBN(_CaseInference, _Handle):
    """AIS-BN (fbn_ais, method 0; the reference's -a 10 stub, src/main.cpp:175-186), mirroring EPISBN:
    max_updates (-m) learning stages of `interval` (-l) samples, each followed by an update of the
    importance CPT of the evidence's unobserved ancestors from the stage's weighted family counts,
    then num_samples (-q) counted samples.  eps: the cutoff in [0, 1), None = the defaults by state
    count.  max_updates=0 is likelihood weighting's draws.  Unbiased; needs no LBP; works on any DAG,
    a disconnected learned network included.  device < 0: the host twin (bit-identical results)."""

    _destroy = "fbn_ais_destroy"
    _method = 0

    def __init__(self, network, num_samples=10000, max_updates=10, interval=2500, eps=None, seed=0, device=0):
        self.network = network
        self.num_samples, self.seed = int(num_samples), int(seed)
        self.max_updates, self.interval = int(max_updates), int(interval)
        self.eps = self._eps_arg(eps)
        self.sum_dom = int(np.sum(network.dims))
        self.stats = None
        h = C.c_void_p()
        lib.fbn_ais_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    @property
    def draws_per_case(self):
        """T: every draw of a case, the learning stages included."""
        if self._method == 0:
            return self.max_updates * self.interval + self.num_samples
        return self.num_samples

    def _run_args(self, n, case_offset):
        return (n, self.num_samples, self.max_updates, self.interval, self.seed, int(case_offset), self.eps)

    def infer(self, evidence, marginals=True, case_offset=0):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (labels, marginals or None);
        self.stats = (log_evidence, ess, updates applied, ess / n of the first stage) per case.
        case_offset: the global index of the first case (a batch split over calls gives the bits of the
        whole batch)."""
        ev, n, labels, marg, st = self._outputs(evidence, marginals, 4)
        lib.fbn_ais_run(self._h, self._method, _p(ev), *self._run_args(n, case_offset), _p(labels), _p(marg), _p(st))
        self.stats = (st[:, 0].copy(), st[:, 1].copy(), st[:, 2].astype(np.int32), st[:, 3].copy())
        return labels, marg

    def run_device(self, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr=None, d_stats_ptr=None, case_offset=0,
                   stream_ptr=None):
        """Device-resident run (one launch, asynchronous on the stream after the evidence check);
        d_stats [ncases][4]."""
        lib.fbn_ais_run_device(self._h, self._method, C.c_void_p(d_evidence_ptr),
                               *self._run_args(int(ncases), case_offset), C.c_void_p(d_labels_ptr),
                               C.c_void_p(d_marg_ptr) if d_marg_ptr else None,
                               C.c_void_p(d_stats_ptr) if d_stats_ptr else None, stream_ptr)

    def debug_samples(self, evidence, case_offset=0):
        """Every draw behind infer(evidence): (values uint8 [V][ncases * T], mantissas fp64, exponents
        int32 [ncases * T], the importance CPT after the last update fp64 [ncases][cells]); draw t of
        case c at c * T + t, T = draws_per_case."""
        ev, n, vals, m, e = self._debug_outputs(evidence, self.draws_per_case)
        icpt = np.zeros((n, self.info()["state_bytes"] // 16), np.float64)
        lib.fbn_ais_debug_samples(self._h, self._method, _p(ev), *self._run_args(n, case_offset), _p(vals), _p(m), _p(e),
                                  _p(icpt))
        return vals, m, e, icpt

    def set_tuning(self, lds_bytes_max=0, max_workgroups=0):
        """fbn_ais_set_tuning: lds_bytes_max < 0 keeps the importance CPT and the counts in a global
        workspace instead of LDS; max_workgroups caps the persistent grid.  0 = default.  Results do not
        change."""
        lib.fbn_ais_set_tuning(self._h, int(lds_bytes_max), int(max_workgroups))

    def info(self, ncases=1):
        """dict(lds_bytes, state_bytes, path, grid): path 0 = the state in LDS, 1 = in global memory;
        grid = the workgroups a run of ncases cases launches."""
        b, sb, p, g = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        lib.fbn_ais_info(self._h, int(ncases), C.byref(b), C.byref(sb), C.byref(p), C.byref(g))
        return {"lds_bytes": b.value, "state_bytes": sb.value, "path": p.value, "grid": g.value}

    def eta(self):
        """The learning rates eta[0 .. max_updates) the runs use (fbn_ais_eta)."""
        out = np.zeros(max(self.max_updates, 1), np.float64)
        lib.fbn_ais_eta(self._method, self.max_updates, _p(out))
        return out[:self.max_updates]

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_ais_last_kernel_ms(self._h, C.byref(ms))
        return ms.value


class SelfImportanceSampling(AISBN):
    """Self-importance sampling (fbn_ais, method 1; the reference's -a 8 stub, src/main.cpp:149-160):
    all num_samples (-q) samples are counted; after each full block of `interval` (-l) samples, while
    samples remain and at most max_updates (-m) times, the importance CPT rows of the evidence's
    unobserved ancestors are replaced by the cumulative weighted frequencies.  It relies on the
    cutoff's floor for support, so eps=0 is refused.  Otherwise as AISBN."""

    _method = 1


class MostProbableExplanation(_Handle):
    """Most probable explanation (fbn_mpe): the complete assignment x* = argmax_x P(x, e) that agrees with
    the evidence, and log P(x*, e) -- exact, by max-product message passing with a back-trace on the
    junction forest, so it takes any DAG.  The value is kept as a mantissa and a binary exponent and
    does not underflow on networks of thousands of variables.  The reference has no counterpart.
    device < 0: the host twin (bit-identical results)."""

    _destroy = "fbn_mpe_destroy"

    def __init__(self, network, device=0):
        self.network = network
        h = C.c_void_p()
        lib.fbn_mpe_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def info(self):
        """dict(cliques, entries, store_rows, components): store_rows = rows of one case's store."""
        c, e, r, k = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        lib.fbn_mpe_info(self._h, C.byref(c), C.byref(e), C.byref(r), C.byref(k))
        return {"cliques": c.value, "entries": e.value, "store_rows": r.value, "components": k.value}

    def value_parts(self, evidence):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (assignment int8 [ncases][num_nodes],
        value fp64 [ncases][2] = (m, ex) with P(x*, e) = m * 2^ex, m in [0.5, 1)).  A case whose value
        underflows inside a clique (m would be 0) raises FastBNError (FBN_ERR_LIMIT) naming it."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        assign = np.zeros((n, self.network.num_nodes), np.int8)
        value = np.zeros((n, 2), np.float64)
        lib.fbn_mpe_run(self._h, _p(ev), n, _p(assign), _p(value))
        return assign, value

    def infer(self, evidence):
        """-> (assignment int8 [ncases][num_nodes], log_p fp64 [ncases] = log P(x*, e))."""
        assign, value = self.value_parts(evidence)
        return assign, np.log(value[:, 0]) + value[:, 1] * np.log(2.0)

    def run_device(self, d_evidence_ptr, ncases, d_assignment_ptr, d_value_ptr, stream_ptr=None):
        """Device-resident run (asynchronous on the stream after the evidence check)."""
        lib.fbn_mpe_run_device(self._h, C.c_void_p(d_evidence_ptr), int(ncases), C.c_void_p(d_assignment_ptr),
                               C.c_void_p(d_value_ptr), stream_ptr)

    def debug_messages(self, evidence):
        """(messages fp64 [ncases][sum of separator entries], exponents int32 [ncases][separators]) as
        Collect leaves them."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        i = self.info()
        nsep = i["cliques"] - i["components"]
        msg = np.zeros((n, i["store_rows"] - nsep - i["cliques"]), np.float64)
        exps = np.zeros((n, nsep), np.int32)
        lib.fbn_mpe_debug_messages(self._h, _p(ev), n, _p(msg), _p(exps))
        return msg, exps

    def set_tuning(self, max_workgroups=0, store_bytes_max=0):
        """fbn_mpe_set_tuning: max_workgroups caps the persistent grid, store_bytes_max the message store
        of all waves together.  0 = default.  Results do not change."""
        lib.fbn_mpe_set_tuning(self._h, int(max_workgroups), int(store_bytes_max))

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_mpe_last_kernel_ms(self._h, C.byref(ms))
        return ms.value


class ExpectationMaximization(_Handle):
    """Parameter learning from incomplete data (fbn_em): expectation-maximisation over the junction forest
    of `network`, whose structure is kept and whose probabilities are the starting parameters.  Data rows
    are int8 [ncases][num_nodes], -1 = missing.  The E-step runs exact junction-tree inference per row (one
    row per GPU lane) and sums the family posteriors; the M-step is (N + pseudo_count) / (T + pseudo_count
    * states).  The reference has no counterpart.  device < 0: the host twin (the same per-case bytes)."""

    _destroy = "fbn_em_destroy"

    def __init__(self, network, pseudo_count=1.0, device=0):
        if not pseudo_count > 0:
            err = FastBNError(f"ExpectationMaximization: the pseudo-count must be > 0 (got {pseudo_count})")
            err.code = -1
            raise err
        self.network_start = network
        self.pseudo_count = float(pseudo_count)
        self.num_nodes = network.num_nodes
        self.dims = network.dims.copy()
        self._npc = [network.node_probs(v)[1].shape[1] for v in range(self.num_nodes)]
        h = C.c_void_p()
        lib.fbn_em_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def info(self):
        """dict(cliques, entries, store_rows, cells, components)."""
        c, e, r, n, k = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        lib.fbn_em_info(self._h, C.byref(c), C.byref(e), C.byref(r), C.byref(n), C.byref(k))
        return {"cliques": c.value, "entries": e.value, "store_rows": r.value, "cells": n.value, "components": k.value}

    def _split(self, flat):
        """the flat cell array as one [dims[v], parent configs] view per node"""
        out, off = [], 0
        for v in range(self.num_nodes):
            n = int(self.dims[v]) * self._npc[v]
            out.append(flat[off:off + n].reshape(int(self.dims[v]), self._npc[v]))
            off += n
        return out

    def estep_flat(self, data):
        """-> (counts fp64 [cells], value fp64 [ncases][2] = (m, ex), P(e) = m * 2^ex)."""
        d = np.ascontiguousarray(data, dtype=np.int8)
        n = d.shape[0]
        counts = np.zeros(self.info()["cells"], np.float64)
        value = np.zeros((n, 2), np.float64)
        lib.fbn_em_estep(self._h, _p(d), n, _p(counts), _p(value))
        return counts, value

    def estep(self, data):
        """One E-step at the current parameters -> (counts: one [dims[v], parent configs] array per node,
        value [ncases][2])."""
        counts, value = self.estep_flat(data)
        return self._split(counts), value

    def estep_device(self, d_data_ptr, ncases, d_counts_ptr, d_value_ptr, stream_ptr=None):
        """Device-resident E-step (asynchronous on the stream after the data check)."""
        lib.fbn_em_estep_device(self._h, C.c_void_p(d_data_ptr), int(ncases), C.c_void_p(d_counts_ptr),
                                C.c_void_p(d_value_ptr) if d_value_ptr else None, stream_ptr)

    def fit(self, data, max_iters=50, tol=1e-6):
        """Iterate E-step and M-step -> objective fp64 [iters_done][2] = (log-likelihood, Q) at the
        parameters each iteration's E-step ran with.  tol = 0 never stops early."""
        d = np.ascontiguousarray(data, dtype=np.int8)
        obj = np.zeros((max(int(max_iters), 1), 2), np.float64)
        done = C.c_int()
        lib.fbn_em_run(self._h, _p(d), d.shape[0], int(max_iters), float(tol), self.pseudo_count, _p(obj), C.byref(done))
        return obj[:done.value].copy()

    def network(self):
        """The current parameters as a probability network."""
        h = C.c_void_p()
        lib.fbn_em_network(self._h, C.byref(h))
        return Network(_handle=h)

    def set_parameters(self, net):
        """Take net's probabilities (same structure, else an error)."""
        lib.fbn_em_set_parameters(self._h, net._h)

    def debug_posteriors(self, data):
        """The per-case family posteriors fp64 [ncases][cells]."""
        d = np.ascontiguousarray(data, dtype=np.int8)
        post = np.zeros((d.shape[0], self.info()["cells"]), np.float64)
        lib.fbn_em_debug_posteriors(self._h, _p(d), d.shape[0], _p(post))
        return post

    def log_likelihood(self, data):
        """log P(e) per case fp64 [ncases] at the current parameters."""
        _, value = self.estep_flat(data)
        return np.log(value[:, 0]) + value[:, 1] * np.log(2.0)

    def set_tuning(self, max_workgroups=0, store_bytes_max=0):
        """fbn_em_set_tuning, as MostProbableExplanation.set_tuning.  Per-case results do not change."""
        lib.fbn_em_set_tuning(self._h, int(max_workgroups), int(store_bytes_max))

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_em_last_kernel_ms(self._h, C.byref(ms))
        return ms.value
