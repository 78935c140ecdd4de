"""halo2_regex_amd — MI355X-native batched DFA witness generator for the halo2-regex chip.

Python here is a thin ctypes binding over the C ABI in include/hrx.h (libhrx.so, built from
halo2_regex_amd/csrc by hipcc for gfx950).  The class and method names mirror the reference's
Rust surface for the path (src/defs.rs, src/table.rs, src/lib.rs:96-113,311-318,766-888) so that the
parity tests read like the reference's own tests.  There is no CPU implementation of the compute
path: without the HIP library the import fails, and without a gfx950 device RegexVerifyConfig raises.
"""
import collections
import contextlib
import ctypes as C
import os

# torch must be imported before libhrx.so: both need libamdhip64.so.7 and the process must end up with
# ONE HIP runtime (torch's bundled copy wins by SONAME when it is loaded first), otherwise device
# pointers of torch tensors would belong to a different runtime than the one launching the kernels.
import torch  # noqa: F401  (plumbing: device memory, streams, torch.distributed)
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HRX_LIB_PATH") or os.path.join(_HERE, "csrc", "libhrx.so")   # (HRX_LIB_PATH: tools/ load the ablation build)

HRX_OK = 0
HRX_ERR_PARSE, HRX_ERR_BOUNDS, HRX_ERR_ARG, HRX_ERR_HIP, HRX_ERR_STATE = 1, 2, 3, 4, 5
HRX_ERR_INVALID_TRANSITION, HRX_ERR_OUT_OF_CONTRACT, HRX_ERR_IO = 6, 7, 8
HRX_DEVICE_SAME = -2                 # hrx_ctx_clone: the source context's device
HRX_DEVICE_NONE = -1                 # hrx_ctx_create: host-only context (the native small-batch host walk)
HRX_DEFAULT_HOST_THRESHOLD = 32768   # rows (B x M) below which host-buffer batches are walked on the host


_u64p = C.POINTER(C.c_uint64)
_u32p = C.POINTER(C.c_uint32)
_u16p = C.POINTER(C.c_uint16)
_u8p = C.POINTER(C.c_uint8)


class _RegexPartC(C.Structure):      # hrx_regex_part of include/hrx.h
    _fields_ = [("regex_def", C.c_char_p), ("regex_len", C.c_size_t), ("is_public", C.c_int), ("max_size", C.c_size_t)]


class _HostRouteReportC(C.Structure):    # hrx_host_route_report of include/hrx.h
    _fields_ = [("route", C.c_int), ("device_strings", C.c_size_t), ("host_strings", C.c_size_t), ("device_ms", C.c_double), ("host_ms", C.c_double), ("call_ms", C.c_double),
                ("device_alone_ns_per_row", C.c_double), ("host_alone_ns_per_row", C.c_double), ("split_ns_per_row", C.c_double),
                ("device_ns_per_row", C.c_double), ("host_ns_per_row", C.c_double), ("host_threads", C.c_int), ("device_pipelined", C.c_int)]


class _ExtractOutC(C.Structure):       # hrx_extract_out of include/hrx.h
    _fields_ = [("run_offsets", C.c_void_p), ("runs", C.c_void_p), ("byte_offsets", C.c_void_p), ("values", C.c_void_p), ("totals", C.c_void_p),
                ("runs_cap", C.c_size_t), ("values_cap", C.c_size_t)]


class _PlaceReportC(C.Structure):    # hrx_place_report of include/hrx.h
    _fields_ = [("searched", C.c_int), ("steps", C.c_int), ("accepted", C.c_int), ("chosen_step", C.c_int),
                ("ref_us", C.c_double), ("first_us", C.c_double), ("best_us", C.c_double),
                ("ref_gbs", C.c_double), ("first_gbs", C.c_double), ("best_gbs", C.c_double), ("probe_bytes", C.c_size_t),
                ("peak_candidate_bytes", C.c_size_t), ("search_ms", C.c_double), ("capped", C.c_int)]


class HrxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "halo2_regex_amd: %s is missing — build it with `make -C halo2_regex_amd/csrc` "
            "(or __graft_entry__.build()); there is no fallback path" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, sz, u64, i = C.c_void_p, C.c_size_t, C.c_uint64, C.c_int
    sig = {
        "hrx_defs_create": (i, [C.POINTER(vp)]),
        "hrx_defs_destroy": (None, [vp]),
        "hrx_defs_push_allstr_text": (i, [vp, C.c_char_p, sz]),
        "hrx_defs_push_allstr_file": (i, [vp, C.c_char_p]),
        "hrx_defs_push_substr_text": (i, [vp, C.c_char_p, sz]),
        "hrx_defs_push_substr_file": (i, [vp, C.c_char_p]),
        "hrx_defs_push_allstr": (i, [vp, u64, u64, u64, sz, _u64p, _u64p, _u8p, _u64p]),
        "hrx_defs_push_substr": (i, [vp, sz, _u64p, _u64p, sz, _u64p, sz, _u64p]),
        "hrx_defs_finalize": (i, [vp]),
        "hrx_defs_num_defs": (sz, [vp]),
        "hrx_defs_num_substrs": (sz, [vp, sz]),
        "hrx_defs_first_state": (u64, [vp, sz]),
        "hrx_defs_accepted_state": (u64, [vp, sz]),
        "hrx_defs_largest_state": (u64, [vp, sz]),
        "hrx_defs_num_transitions": (sz, [vp, sz]),
        "hrx_defs_substr_id_offset": (u64, [vp, sz]),
        "hrx_defs_table_bytes": (sz, [vp]),
        "hrx_table_transition_rows": (sz, [vp, sz, _u64p, sz]),
        "hrx_table_endpoint_rows": (sz, [vp, sz, _u64p, sz]),
        "hrx_device_count": (i, [C.POINTER(i)]),
        "hrx_ctx_create": (i, [vp, i, C.POINTER(vp)]),
        "hrx_ctx_destroy": (None, [vp]),
        "hrx_ctx_device": (i, [vp]),
        "hrx_ctx_clone": (i, [vp, i, C.POINTER(vp)]),
        "hrx_ctx_set_host_threshold": (i, [vp, sz]),
        "hrx_ctx_host_threshold": (sz, [vp]),
        "hrx_ctx_set_placement": (i, [vp, i, sz, C.c_double]),
        "hrx_last_error": (C.c_char_p, []),
        "hrx_witness_batch_device": (i, [vp, vp, sz, vp, sz, sz, vp, vp, vp, vp]),
        "hrx_witness_batch_device_pitched": (i, [vp, vp, sz, vp, sz, sz, vp, sz, vp, sz, vp, vp]),
        "hrx_recommended_pitches": (None, [sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]),
        "hrx_witness_batch_device_layout": (i, [vp, i, vp, sz, vp, sz, sz, vp, vp, vp, vp]),
        "hrx_position_major_sizes": (None, [sz, sz, sz, C.POINTER(sz), C.POINTER(sz)]),
        "hrx_witness_batch_device_planes": (i, [vp, i, vp, sz, vp, sz, sz, C.POINTER(vp), sz, vp, vp, vp]),
        "hrx_position_major_plane_sizes": (None, [sz, sz, C.POINTER(sz), C.POINTER(sz)]),
        "hrx_position_major_stripe_sizes": (None, [sz, sz, sz, C.POINTER(sz), C.POINTER(sz)]),
        "hrx_alloc_output_planes": (i, [vp, sz, sz, sz, C.POINTER(vp), C.POINTER(vp)]),
        "hrx_alloc_output_planes_for_batch": (i, [vp, i, vp, sz, vp, sz, sz, sz, C.POINTER(vp), C.POINTER(vp)]),
        "hrx_rows_of_string_planes": (i, [C.POINTER(vp), sz, vp, sz, sz, sz, sz, vp, vp]),
        "hrx_probe_write_pair": (i, [vp, vp, vp, sz, C.POINTER(C.c_double)]),
        "hrx_traffic_pass_device_planes": (i, [vp, vp, sz, sz, sz, C.POINTER(vp), sz, vp, vp]),
        "hrx_witness_of_string": (i, [vp, sz, sz, sz, vp, vp, vp, vp]),
        "hrx_witness_num_columns": (sz, [sz]),
        "hrx_witness_columns_host": (i, [i, vp, sz, vp, vp, sz, vp, sz, sz, sz, sz, sz, sz, vp]),
        "hrx_ctx_host_route_report": (i, [vp, C.POINTER(_HostRouteReportC), sz]),
        "hrx_alloc_last_report_sized": (i, [vp, vp, sz]),
        "hrx_ctx_set_option": (i, [vp, i, C.c_long]),
        "hrx_ctx_get_option": (C.c_long, [vp, i]),
        "hrx_rows_of_string_position_major": (i, [vp, vp, sz, sz, sz, sz, vp, vp]),
        "hrx_describe_launch": (i, [vp, i, sz, sz, i, C.c_char_p, sz]),
        "hrx_ctx_describe_launch": (i, [vp, i, sz, sz, C.c_char_p, sz]),
        "hrx_alloc_outputs_position_major": (i, [vp, sz, sz, C.POINTER(vp), C.POINTER(vp)]),
        "hrx_alloc_output_pair": (i, [vp, sz, sz, C.POINTER(vp), C.POINTER(vp)]),
        "hrx_device_free": (i, [vp]),
        "hrx_alloc_last_report": (i, [vp, C.POINTER(_PlaceReportC)]),
        "hrx_traffic_pass_device": (i, [vp, vp, sz, sz, sz, vp, vp, vp]),
        "hrx_traffic_pass_device_layout": (i, [vp, i, vp, sz, sz, sz, vp, sz, vp, sz, vp]),
        "hrx_chars_to_position_major_device": (i, [vp, vp, sz, sz, vp, vp]),
        "hrx_multi_create": (i, [vp, C.POINTER(i), i, C.POINTER(vp)]),
        "hrx_multi_destroy": (None, [vp]),
        "hrx_multi_num_shards": (i, [vp]),
        "hrx_multi_shard_device": (i, [vp, i]),
        "hrx_multi_shard_stream": (vp, [vp, i]),
        "hrx_multi_witness_batch_device": (i, [vp, i, C.POINTER(vp), sz, C.POINTER(vp), C.POINTER(sz), sz, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
        "hrx_multi_synchronize": (i, [vp]),
        "hrx_multi_witness_batch_host": (i, [vp, _u8p, sz, _u32p, sz, sz, _u32p, _u16p, _u64p]),
        "hrx_fr_num_columns": (sz, [sz]),
        "hrx_fr_columns_device": (i, [vp, i, vp, sz, vp, vp, sz, vp, sz, sz, sz, sz, sz, vp, i, vp]),
        "hrx_fr_columns_device_planes": (i, [vp, i, vp, sz, vp, C.POINTER(vp), sz, vp, sz, sz, sz, sz, vp, i, vp]),
        "hrx_fr_from_u64": (None, [C.c_uint64, i, _u64p]),
        "hrx_verify_rows_device": (i, [vp, i, vp, sz, vp, vp, sz, vp, sz, sz, sz, vp, vp]),
        "hrx_verify_rows_device_planes": (i, [vp, i, vp, sz, vp, C.POINTER(vp), sz, vp, sz, sz, vp, vp]),
        "hrx_verify_rows_host": (i, [vp, i, vp, sz, vp, vp, sz, vp, sz, sz, sz, vp]),
        "hrx_verify_chunked_workspace_bytes": (sz, [sz, sz, sz]),
        "hrx_ctx_verify_chunk_rows": (sz, [vp, sz, sz]),
        "hrx_verify_rows_chunked_device": (i, [vp, i, vp, sz, vp, vp, sz, vp, sz, sz, sz, sz, vp, sz, vp, vp]),
        "hrx_verify_rows_chunked_device_planes": (i, [vp, i, vp, sz, vp, C.POINTER(vp), sz, vp, sz, sz, sz, vp, sz, vp, vp]),
        "hrx_verify_rows_chunked_host": (i, [vp, i, vp, sz, vp, vp, sz, vp, sz, sz, sz, sz, vp]),
        "hrx_lookup_words_per_string": (sz, [vp]),
        "hrx_lookup_layout": (i, [vp, sz] + [C.POINTER(sz)] * 5),
        "hrx_lookup_counts_device": (i, [vp, i, vp, sz, vp, vp, sz, sz, sz, sz, sz, vp, vp, vp]),
        "hrx_lookup_counts_device_planes": (i, [vp, i, vp, sz, vp, C.POINTER(vp), sz, sz, sz, sz, sz, vp, vp, vp]),
        "hrx_lookup_counts_host": (i, [vp, i, vp, sz, vp, vp, sz, sz, sz, sz, sz, vp, vp]),
        "hrx_ctx_lookup_group": (i, [vp, sz, C.POINTER(sz), C.POINTER(sz)]),
        "hrx_lookup_num_columns": (sz, [sz]),
        "hrx_lookup_compress_inputs_device": (i, [vp, i, vp, sz, vp, vp, sz, sz, sz, sz, sz, vp, sz, vp, i, vp]),
        "hrx_lookup_compress_inputs_device_planes": (i, [vp, i, vp, sz, vp, C.POINTER(vp), sz, sz, sz, sz, sz, vp, sz, vp, i, vp]),
        "hrx_lookup_compress_inputs_host": (i, [vp, i, vp, sz, vp, vp, sz, sz, sz, sz, sz, vp, sz, vp, i]),
        "hrx_lookup_compress_table_device": (i, [vp, vp, sz, sz, vp, i, vp]),
        "hrx_lookup_compress_table_host": (i, [vp, vp, sz, sz, vp, i]),
        "hrx_fr_mul": (None, [_u64p, _u64p, _u64p]),
        "hrx_lookup_permute_workspace_bytes": (sz, [vp, sz, sz]),
        "hrx_lookup_permute_device": (i, [vp, vp, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp, sz, vp]),
        "hrx_lookup_permute_host": (i, [vp, vp, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp]),
        "hrx_ctx_lookup_permute_plan": (i, [vp, sz, sz] + [C.POINTER(sz)] * 4),
        "hrx_lookup_invert_workspace_bytes": (sz, [vp, sz]),
        "hrx_lookup_invert_table_device": (i, [vp, vp, sz, vp, sz, vp, i, vp, sz, vp]),
        "hrx_lookup_invert_table_host": (i, [vp, vp, sz, vp, sz, vp, i]),
        "hrx_lookup_product_device": (i, [vp, vp, sz, sz, sz, vp, vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, sz, vp, sz, vp, i, vp]),
        "hrx_lookup_product_host": (i, [vp, vp, sz, sz, sz, vp, vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, sz, vp, sz, vp, i]),
        "hrx_ctx_lookup_product_plan": (i, [vp, sz, sz] + [C.POINTER(sz)] * 2),
        "hrx_fr_ntt_workspace_bytes": (sz, [C.c_uint]),
        "hrx_fr_ntt_prepare_device": (i, [vp, C.c_uint, vp, sz, vp]),
        "hrx_fr_ntt_device": (i, [vp, vp, sz, vp, sz, sz, C.c_uint, sz, vp, i, vp, sz, vp]),
        "hrx_fr_ntt_host": (i, [vp, vp, sz, vp, sz, sz, C.c_uint, sz, vp, i]),
        "hrx_ctx_fr_ntt_plan": (i, [vp, sz, C.c_uint, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]),
        "hrx_fr_sub": (None, [_u64p, _u64p, _u64p]),
        "hrx_fr_vanishing_inverse_device": (i, [vp, C.c_uint, C.c_uint, vp, vp, i, vp]),
        "hrx_fr_vanishing_inverse_host": (i, [vp, C.c_uint, C.c_uint, vp, vp, i]),
        "hrx_lookup_quotient_device": (i, [vp, sz, C.c_uint, C.c_uint, vp, vp, vp, vp, sz, vp, sz, sz, vp, sz, vp, vp, vp, sz, vp, vp, sz, vp, i, vp]),
        "hrx_lookup_quotient_host": (i, [vp, sz, C.c_uint, C.c_uint, vp, vp, vp, vp, sz, vp, sz, sz, vp, sz, vp, vp, vp, sz, vp, vp, sz, vp, i]),
        "hrx_ctx_lookup_quotient_plan": (i, [vp, sz, C.c_uint, C.POINTER(sz), C.POINTER(sz)]),
        "hrx_witness_batch_host": (i, [vp, _u8p, sz, _u32p, sz, sz, _u32p, _u16p, _u64p]),
        "hrx_match_batch_device": (i, [vp, i, vp, sz, vp, sz, sz, vp, vp, vp, sz, vp]),
        "hrx_match_batch_host": (i, [vp, _u8p, sz, _u32p, sz, sz, _u64p, _u32p, _u64p, sz]),
        "hrx_describe_match": (i, [vp, i, sz, sz, i, C.c_char_p, sz]),
        "hrx_ctx_describe_match": (i, [vp, i, sz, sz, C.c_char_p, sz]),
        "hrx_match_batch_device_ragged": (i, [vp, vp, vp, sz, sz, vp, vp, vp, sz, vp]),
        "hrx_match_batch_host_ragged": (i, [vp, _u8p, _u64p, sz, sz, _u64p, _u32p, _u64p, sz]),
        "hrx_ragged_to_position_major_device": (i, [vp, vp, vp, sz, sz, vp, vp, vp]),
        "hrx_extract_workspace_bytes": (sz, [sz]),
        "hrx_extract_spans_device": (i, [vp, i, vp, sz, vp, sz, vp, vp, vp, sz, C.c_uint32, C.POINTER(_ExtractOutC), vp, sz, vp]),
        "hrx_extract_spans_host": (i, [i, vp, sz, vp, sz, vp, vp, vp, sz, C.c_uint32, C.POINTER(_ExtractOutC), i]),
        "hrx_route_workspace_bytes": (sz, [sz]),
        "hrx_route_device": (i, [vp, vp, C.c_uint32, vp, vp, sz, _u32p, sz, vp, vp, vp, sz, vp]),
        "hrx_route_host": (i, [vp, C.c_uint32, vp, vp, sz, _u32p, sz, vp, vp]),
        "hrx_gather_to_position_major_device": (i, [vp, i, vp, sz, vp, vp, sz, vp, sz, sz, vp, vp, vp]),
        "hrx_match_selected_device": (i, [vp, i, vp, sz, vp, vp, sz, vp, sz, sz, vp, vp, vp, sz, vp]),
        "hrx_match_selected_host": (i, [vp, i, vp, sz, vp, vp, sz, vp, sz, sz, vp, vp, vp, sz]),
        "hrx_shard_range": (None, [sz, i, i, C.POINTER(sz), C.POINTER(sz)]),
        "hrx_derive_states": (i, [vp, _u8p, sz, _u64p]),
        "hrx_derive_substr_ids": (i, [vp, _u64p, sz, _u64p]),
        "hrx_derive_is_start_end": (i, [vp, _u64p, _u64p, sz, _u8p, _u8p]),
        "hrx_match_substrs": (i, [vp, _u8p, sz, sz] + [_u64p] * 9),
        "hrx_regex_to_allstr_text": (i, [C.c_char_p, sz, C.c_char_p, sz, C.POINTER(sz)]),
        "hrx_regex_to_dfa_json": (i, [C.c_char_p, sz, C.c_char_p, sz, C.POINTER(sz)]),
        "hrx_gen_regex_files": (i, [C.POINTER(_RegexPartC), sz, sz, C.POINTER(vp)]),
        "hrx_regex_files_num_substrs": (sz, [vp]),
        "hrx_regex_files_allstr": (vp, [vp, C.POINTER(sz)]),
        "hrx_regex_files_substr": (vp, [vp, sz, C.POINTER(sz)]),
        "hrx_regex_files_destroy": (None, [vp]),
        "hrx_format_regex_str": (i, [C.c_char_p, sz, C.c_char_p, sz, C.POINTER(sz)]),
        "hrx_regex_find": (i, [C.c_char_p, sz, C.c_char_p, sz, C.POINTER(i), C.POINTER(sz), C.POINTER(sz)]),
    }
    _load.symbols = list(sig)
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    if hasattr(lib, "hrx_chunked_alloc"):      # tools builds only (libhrx_ablation.so: csrc/hrx_alloc.cpp, the placement probes)
        lib.hrx_chunked_alloc.restype, lib.hrx_chunked_alloc.argtypes = i, [i, sz, C.POINTER(vp)]
        lib.hrx_chunked_free.restype, lib.hrx_chunked_free.argtypes = i, [vp]
    return lib


lib = _load()
#: every symbol include/hrx.h declares = every symbol bound above (tests check that the header, this list and the library's exports agree)
ABI_SYMBOLS = list(_load.symbols)


class DeviceBuffer:
    """TOOLS ONLY (needs libhrx_ablation.so): `nbytes` of device memory from csrc/hrx_alloc.cpp — a virtual range over 2-MiB
    physical chunks, for the placement probes of DESIGN.md §6 — exposed through __cuda_array_interface__; freed with the object."""

    def __init__(self, nbytes, device=0):
        if not hasattr(lib, "hrx_chunked_alloc"):
            raise HrxError(HRX_ERR_STATE, "DeviceBuffer needs the tools build: HRX_LIB_PATH=.../libhrx_ablation.so")
        p = C.c_void_p()
        _check(lib.hrx_chunked_alloc(int(device), int(nbytes), C.byref(p)))
        self.ptr, self.nbytes, self.device = p.value, int(nbytes), int(device)
        self.__cuda_array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 2}

    def tensor(self, dtype=None):
        """a torch view of the whole buffer (keeps this object alive)"""
        t = torch.as_tensor(self, device=torch.device("cuda", self.device))
        return t if dtype is None else t.view(dtype)

    def __del__(self):
        if getattr(self, "ptr", None) and lib is not None:      # (lib is None while the interpreter shuts down)
            lib.hrx_chunked_free(self.ptr)
            self.ptr = None


class _LibraryOwned:
    """device memory handed out by the library (hrx_alloc_outputs_position_major), as a __cuda_array_interface__ object: the
    torch tensors made from it keep it alive, hrx_device_free runs when the last of them goes"""

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, int(nbytes)
        self.__cuda_array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 2}

    def __del__(self):
        if getattr(self, "ptr", None) and lib is not None:
            lib.hrx_device_free(self.ptr)
            self.ptr = None


def device_empty(numel, dtype, device, chunked=False):
    """torch.empty((numel,), dtype) on `device`; chunked=True (tools only): backed by a DeviceBuffer"""
    dev = torch.device(device)
    if not chunked:
        return torch.empty((int(numel),), dtype=dtype, device=dev)
    nbytes = max(int(numel) * torch.empty((), dtype=dtype).element_size(), 1)
    return DeviceBuffer(nbytes, dev.index if dev.index is not None else torch.cuda.current_device()).tensor(dtype)[:numel]


def _check(rc):
    if rc != HRX_OK:
        raise HrxError(rc, lib.hrx_last_error().decode("utf-8", "replace"))


def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _ptr(a, t):
    return a.ctypes.data_as(t)


# ---------------------------------------------------------------------------------------------
# definition generation — src/vrm/mod.rs, src/vrm/js_caller.rs, src/vrm/regex.js (host only)
# ---------------------------------------------------------------------------------------------
def _two_call(fn, regex):
    data = regex.encode("utf-8") if isinstance(regex, str) else bytes(regex)
    need = C.c_size_t(0)
    _check(fn(data, len(data), None, 0, C.byref(need)))
    buf = C.create_string_buffer(max(need.value, 1))
    _check(fn(data, len(data), buf, need.value, C.byref(need)))
    return buf.raw[:need.value]


def get_dfa_json_value(regex):
    """get_dfa_json_value (src/vrm/js_caller.rs:43-48): the minimal DFA of `regex` as the parsed JSON value
    regexToDfa returns — computed natively, no JS engine."""
    import json
    return json.loads(_two_call(lib.hrx_regex_to_dfa_json, regex).decode("utf-8"))


def regex_to_dfa_json_text(regex):
    return _two_call(lib.hrx_regex_to_dfa_json, regex).decode("utf-8")


def regex_to_allstr_text(regex):
    """regexToDfa + dfa_to_regex_def_text (src/vrm/js_caller.rs:127-157): the AllstrRegexDef text of `regex`."""
    return _two_call(lib.hrx_regex_to_allstr_text, regex).decode("ascii")


def format_regex_str(regex):
    """format_regex_str (src/vrm/js_caller.rs:36-41): formatRegexPrintable of src/vrm/regex.js:24-39."""
    return _two_call(lib.hrx_format_regex_str, regex).decode("utf-8")


def regex_find(pattern, text):
    """The leftmost-first search gen_regex_files runs for every part on every DFA path (mod.rs:553-583);
    returns (start, end) or None."""
    p = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
    t = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    found, s0, e0 = C.c_int(0), C.c_size_t(0), C.c_size_t(0)
    _check(lib.hrx_regex_find(p, len(p), t, len(t), C.byref(found), C.byref(s0), C.byref(e0)))
    return (s0.value, e0.value) if found.value else None


class RegexPartConfig:
    """RegexPartConfig (src/vrm/mod.rs:39-49)."""

    def __init__(self, is_public, regex_def, max_size, solidity=None):
        self.is_public, self.regex_def, self.max_size, self.solidity = bool(is_public), regex_def, int(max_size), solidity


class DecomposedRegexConfig:
    """DecomposedRegexConfig (src/vrm/mod.rs:31-37): gen_regex_files (mod.rs:62-307) computed natively — the
    AllstrRegexDef text of the concatenated parts and one SubstrRegexDef text per public part."""

    def __init__(self, max_byte_size, parts):
        self.max_byte_size, self.parts = int(max_byte_size), list(parts)

    @classmethod
    def from_json(cls, text):
        import json
        v = json.loads(text)
        return cls(v["max_byte_size"], [RegexPartConfig(p["is_public"], p["regex_def"], p["max_size"], p.get("solidity"))
                                       for p in v["parts"]])

    def all_regex(self):
        return "".join(p.regex_def for p in self.parts)   # mod.rs:87-91

    def gen_allstr_text(self):
        return regex_to_allstr_text(self.all_regex())

    def gen_allstr_file(self, allstr_file_path):
        with open(allstr_file_path, "w") as f:
            f.write(self.gen_allstr_text())

    def gen_regex_texts(self):
        """-> (allstr_text, [substr_text per public part])"""
        keep = [p.regex_def.encode("utf-8") for p in self.parts]
        arr = (_RegexPartC * max(len(keep), 1))()
        for k, (p, b) in enumerate(zip(self.parts, keep)):
            arr[k] = _RegexPartC(b, len(b), int(p.is_public), p.max_size)
        h = C.c_void_p()
        _check(lib.hrx_gen_regex_files(arr, len(keep), self.max_byte_size, C.byref(h)))
        try:
            n = C.c_size_t(0)
            ptr = lib.hrx_regex_files_allstr(h, C.byref(n))
            allstr = C.string_at(ptr, n.value).decode("ascii")
            subs = []
            for k in range(lib.hrx_regex_files_num_substrs(h)):
                ptr = lib.hrx_regex_files_substr(h, k, C.byref(n))
                subs.append(C.string_at(ptr, n.value).decode("ascii"))
        finally:
            lib.hrx_regex_files_destroy(h)
        return allstr, subs

    def gen_regex_files(self, allstr_file_path, substr_file_pathes):
        """gen_regex_files (mod.rs:62-307): writes the AllstrRegexDef file and one SubstrRegexDef file per public part."""
        allstr, subs = self.gen_regex_texts()
        if len(substr_file_pathes) < len(subs):
            raise ValueError("%d public parts but %d substr paths" % (len(subs), len(substr_file_pathes)))
        with open(allstr_file_path, "w") as f:
            f.write(allstr)
        for path, text in zip(substr_file_pathes, subs):
            with open(path, "w") as f:
                f.write(text)


# ---------------------------------------------------------------------------------------------
# data model — src/defs.rs
# ---------------------------------------------------------------------------------------------
class AllstrRegexDef:
    """AllstrRegexDef (src/defs.rs:26-36): holds the definition text; parsing happens in C."""

    def __init__(self, text):
        self.text = text.encode() if isinstance(text, str) else bytes(text)

    @classmethod
    def read_from_text(cls, file_path):  # defs.rs:54-58
        with open(file_path, "rb") as f:
            return cls(f.read())


class SubstrRegexDef:
    """SubstrRegexDef (src/defs.rs:115-132)."""

    def __init__(self, text):
        self.text = text.encode() if isinstance(text, str) else bytes(text)

    @classmethod
    def read_from_text(cls, file_path):  # defs.rs:184-188
        with open(file_path, "rb") as f:
            return cls(f.read())

    @classmethod
    def new(cls, max_length, min_position, max_position, valid_state_transitions, start_states, end_states):
        """SubstrRegexDef::new (defs.rs:147-163), rendered to the text format of defs.rs:165-177."""
        lines = [str(max_length), str(min_position), str(max_position),
                 " ".join(str(s) for s in start_states), " ".join(str(s) for s in end_states)]
        lines += ["%d %d" % (a, b) for a, b in sorted(valid_state_transitions)]
        return cls("\n".join(lines) + "\n")


class RegexDefs:
    """RegexDefs { allstr, substrs } (src/defs.rs:17-22)."""

    def __init__(self, allstr, substrs):
        self.allstr = allstr
        self.substrs = list(substrs)


class _DefsHandle:
    def __init__(self, regex_defs):
        self.h = C.c_void_p()
        _check(lib.hrx_defs_create(C.byref(self.h)))
        try:
            for rd in regex_defs:
                _check(lib.hrx_defs_push_allstr_text(self.h, rd.allstr.text, len(rd.allstr.text)))
                for sd in rd.substrs:
                    _check(lib.hrx_defs_push_substr_text(self.h, sd.text, len(sd.text)))
            _check(lib.hrx_defs_finalize(self.h))
        except Exception:
            lib.hrx_defs_destroy(self.h)
            self.h = None
            raise

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:   # (module globals are gone at interpreter shutdown)
            lib.hrx_defs_destroy(self.h)
            self.h = None


class RegexTableConfig:
    """The integer rows RegexTableConfig::load assigns (src/table.rs:61-198)."""

    def __init__(self, defs_handle, def_idx):
        self._d = defs_handle
        self.def_idx = def_idx

    def transition_rows(self):
        n = lib.hrx_table_transition_rows(self._d.h, self.def_idx, None, 0)
        rows = np.zeros((n, 4), np.uint64)
        lib.hrx_table_transition_rows(self._d.h, self.def_idx, _ptr(rows, _u64p), n)
        return rows

    def endpoint_rows(self):
        n = lib.hrx_table_endpoint_rows(self._d.h, self.def_idx, None, 0)
        rows = np.zeros((n, 3), np.uint64)
        lib.hrx_table_endpoint_rows(self._d.h, self.def_idx, _ptr(rows, _u64p), n)
        return rows


class AssignedRegexResult:
    """Integer content of AssignedRegexResult (src/lib.rs:79-93) plus the per-def advice columns."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def device_count():
    n = C.c_int(0)
    _check(lib.hrx_device_count(C.byref(n)))
    return n.value


def recommended_pitches(M):
    """(records pitch, masked pitch) in rows and an input stride in bytes that keep the write/read fronts off a
    power-of-two stride (hrx_recommended_pitches)."""
    a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    lib.hrx_recommended_pitches(M, C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


LAYOUT_STRING_MAJOR, LAYOUT_POSITION_MAJOR, LAYOUT_INPUT_POSITION_MAJOR = 0, 1, 2
LAYOUT_RECORD_PLANES = 4      # describe_launch only: the launch witness_batch_planes makes
LAYOUT_INPUT_RAGGED = 8       # describe_match only: the launch match_batch_ragged makes (values + offsets, include/hrx.h RAGGED)
LAYOUT_INPUT_SELECTED = 16    # describe_match only, or-ed with LAYOUT_STRING_MAJOR or LAYOUT_INPUT_RAGGED: the launch match_selected makes, B = len(sel)


PLACE_OFF, PLACE_WALK = 0, 1     # hrx_ctx_set_placement modes
OPT_PMD_COMBINER_WAVE = 1        # hrx_ctx_set_option: 0 default, 1 on, 2 off
OPT_HOST_ROUTE, OPT_HOST_THREADS, OPT_HOST_PIPELINE, OPT_PLACE_DRY_LAUNCH = 2, 3, 4, 5
OPT_MATCH_FUSED_WIDE = 6      # match entry points, four to eight defs: 1 = the fused walk on the class-wide tables where the plan allows it (include/hrx.h)
HOST_ROUTE_AUTO, HOST_ROUTE_DEVICE, HOST_ROUTE_HOST = 0, 1, 2
PLACE_CAPPED_STEPS, PLACE_CAPPED_BYTES, PLACE_CAPPED_TIME, PLACE_CAPPED_ALLOC = 1, 2, 4, 8      # hrx_place_report.capped
PLACED_FROM = 128 << 20    # alloc_outputs*: records of this many bytes or more come from the library's placement-aware allocator (kPlaceFromBytes)
PM_BLOCK = 65536          # kPmBlock of csrc/hrx_lane.h: position-major buffers are blocked by this many strings


def _cat(parts):
    return parts[0] if len(parts) == 1 else (torch.cat(parts) if hasattr(parts[0], "permute") else np.concatenate(parts))


def chars_to_position_major(chars):
    """(B, stride) bytes, stride % 16 == 0  ->  flat HRX_LAYOUT_INPUT_POSITION_MAJOR buffer: per block of PM_BLOCK strings
    [stride/16][nb][16], blocks back to back (one block = the plain layout for B <= PM_BLOCK); torch or numpy."""
    B, stride = chars.shape
    if hasattr(chars, "is_cuda") and chars.is_cuda:       # written block by block into the one output buffer (no second copy of the batch)
        out = torch.empty((B * stride,), dtype=chars.dtype, device=chars.device)
        for k0 in range(0, B, PM_BLOCK):
            c = chars[k0:k0 + PM_BLOCK]
            nb = c.shape[0]
            out[k0 * stride:(k0 + nb) * stride].view(stride // 16, nb, 16).copy_(c.reshape(nb, stride // 16, 16).permute(1, 0, 2))
        return out
    parts = []
    for k0 in range(0, B, PM_BLOCK):
        c = chars[k0:k0 + PM_BLOCK]
        c = c.reshape(c.shape[0], stride // 16, 16)
        c = c.permute(1, 0, 2).contiguous() if hasattr(c, "permute") else np.ascontiguousarray(c.transpose(1, 0, 2))
        parts.append(c.reshape(-1))
    return _cat(parts)


def position_major_to_string_major(records_pm, masked_pm, B, M, D):
    """Inverse of HRX_LAYOUT_POSITION_MAJOR (include/hrx.h): per block of PM_BLOCK strings records [ceil(M/4)][D][nb][4] ->
    (nb, M, D), masked [ceil(M/8)][nb][8] -> (nb, M); returns (B, M, D) and (B, M).  Works on torch tensors and numpy arrays
    alike; no values change (a view for a single block)."""
    q4, q8 = (M + 3) // 4, (M + 7) // 8
    recs, msks = [], []
    for k0 in range(0, B, PM_BLOCK):
        nb = min(PM_BLOCK, B - k0)
        r = records_pm[k0 * q4 * 4 * D:(k0 + nb) * q4 * 4 * D].reshape(q4, D, nb, 4)
        m = masked_pm[k0 * q8 * 8:(k0 + nb) * q8 * 8].reshape(q8, nb, 8)
        r = r.permute(2, 0, 3, 1) if hasattr(r, "permute") else r.transpose(2, 0, 3, 1)      # (nb, M/4, 4, D)
        m = m.permute(1, 0, 2) if hasattr(m, "permute") else m.transpose(1, 0, 2)
        recs.append(r.reshape(nb, -1, D)[:, :M])
        msks.append(m.reshape(nb, -1)[:, :M])
    return _cat(recs), _cat(msks)


def rows_of_string_position_major(records_pm, masked_pm, B, M, D, b, out=None):
    """hrx_rows_of_string_position_major: one circuit's rows — (M, D) uint32 records and (M,) uint16 masked rows of string b — gathered on the host out of
    position-major HOST arrays (numpy; e.g. the device buffers copied out as they are)."""
    rec = np.empty((M, D), np.uint32) if out is None else out[0]
    msk = np.empty(M, np.uint16) if out is None else out[1]
    rp = np.ascontiguousarray(records_pm).view(np.uint32)
    mp = np.ascontiguousarray(masked_pm).view(np.uint16)
    _check(lib.hrx_rows_of_string_position_major(rp.ctypes.data, mp.ctypes.data, B, M, D, b, rec.ctypes.data, msk.ctypes.data))
    return rec, msk


def planes_to_string_major(planes, masked_pm, B, M, D=None):
    """Inverse of the record-planes layout (include/hrx.h hrx_witness_batch_device_planes): the D planes — each per block of PM_BLOCK strings [ceil(M/4)][nb][4] — or, D = 1 with two
    buffers, the two ROW STRIPES of the one def (quad q in buffer q % 2 at slot q / 2), and the position-major masked rows -> (B, M, D) and (B, M); torch tensors or numpy arrays."""
    D = len(planes) if D is None else D
    R = len(planes) // D
    q4, q8 = (M + 3) // 4, (M + 7) // 8
    slots = (q4 + R - 1) // R
    is_t = hasattr(planes[0], "permute")
    recs, msks = [], []
    for k0 in range(0, B, PM_BLOCK):
        nb = min(PM_BLOCK, B - k0)
        per_def = []
        for d in range(D):
            quads = []      # (slots, nb, 4) per stripe -> interleave the stripes' slots back into quad order
            for r in range(R):
                x = planes[r * D + d][k0 * slots * 4:(k0 + nb) * slots * 4].reshape(slots, nb, 4)
                quads.append(x)
            if R == 1:
                q = quads[0]
            else:
                q = (torch.stack(quads, dim=1) if is_t else np.stack(quads, axis=1)).reshape(slots * R, nb, 4)[:q4]
            q = q.permute(1, 0, 2) if is_t else q.transpose(1, 0, 2)            # (nb, q4, 4)
            per_def.append(q.reshape(nb, -1)[:, :M])
        recs.append(torch.stack(per_def, dim=2) if is_t else np.stack(per_def, axis=2))
        m = masked_pm[k0 * q8 * 8:(k0 + nb) * q8 * 8].reshape(q8, nb, 8)
        m = m.permute(1, 0, 2) if is_t else m.transpose(1, 0, 2)
        msks.append(m.reshape(nb, -1)[:, :M])
    return _cat(recs), _cat(msks)


def rows_of_string_planes(planes, masked_pm, B, M, b, out=None, D=None):
    """hrx_rows_of_string_planes: one circuit's rows out of record planes (or the two row stripes of one def: D=1) in HOST memory (numpy arrays, each buffer copied from the device as it is)."""
    D = len(planes) if D is None else D
    rec = np.empty((M, D), np.uint32) if out is None else out[0]
    msk = np.empty(M, np.uint16) if out is None else out[1]
    ps = [np.ascontiguousarray(p).view(np.uint32) for p in planes]
    arr = (C.c_void_p * len(ps))(*[p.ctypes.data for p in ps])
    mp = np.ascontiguousarray(masked_pm).view(np.uint16)
    _check(lib.hrx_rows_of_string_planes(arr, len(ps), mp.ctypes.data, B, M, D, b, rec.ctypes.data, msk.ctypes.data))
    return rec, msk


def witness_of_string(records, n):
    """hrx_witness_of_string: (states (D, n+1) uint64, substr_ids (D, n) uint64, is_starts (D, n+1) bool, is_ends (D, n+1) bool) — what lib.rs:316-318 derive —
    out of one string's compact records, a (M, D) uint32 array."""
    rec = np.ascontiguousarray(records).view(np.uint32)
    M, D = rec.shape
    states, sids = np.zeros((D, n + 1), np.uint64), np.zeros((D, n), np.uint64)      # (usize == u64 on every target of this library)
    st, en = np.zeros((D, n + 1), np.uint8), np.zeros((D, n + 1), np.uint8)
    _check(lib.hrx_witness_of_string(rec.ctypes.data, D, n, M, states.ctypes.data, sids.ctypes.data, st.ctypes.data, en.ctypes.data))
    return states, sids, st.astype(bool), en.astype(bool)


def witness_columns_host(chars, lens, records, masked, M, D, b_begin=0, b_count=None, position_major=False, chars_pm_stride=None, B=None):
    """hrx_witness_columns_host: (4 + 4 D, b_count, M) uint64 — the integer content of every advice column of circuits [b_begin, b_begin + b_count) out of a finished batch
    in host memory (numpy): string-major records (B, M, D) / masked (B, M) / chars (B, stride), or the flat position-major buffers with position_major=True."""
    lens = np.ascontiguousarray(lens, np.uint32)
    B = len(lens) if B is None else B
    b_count = B - b_begin if b_count is None else b_count
    cols = np.empty((4 + 4 * D, b_count, M), np.uint64)
    rec, msk, ch = np.ascontiguousarray(records).view(np.uint32), np.ascontiguousarray(masked).view(np.uint16), np.ascontiguousarray(chars)
    if position_major:
        layout = LAYOUT_POSITION_MAJOR | (LAYOUT_INPUT_POSITION_MAJOR if chars_pm_stride else 0)
        stride = int(chars_pm_stride) if chars_pm_stride else ch.shape[1]
        rp = mp = 0
    else:
        layout, stride, rp, mp = LAYOUT_STRING_MAJOR, ch.shape[1], rec.strides[0] // (4 * D), msk.strides[0] // 2
    _check(lib.hrx_witness_columns_host(layout, ch.ctypes.data, stride, lens.ctypes.data, rec.ctypes.data, rp, msk.ctypes.data, mp, B, M, D, b_begin, b_count, cols.ctypes.data))
    return cols


def shard_range(B, world, rank):
    b, c = C.c_size_t(0), C.c_size_t(0)
    lib.hrx_shard_range(B, world, rank, C.byref(b), C.byref(c))
    return b.value, c.value


def _torch_row_pitches(chars, records, masked, layout, D, rec_pitch, msk_pitch, chars_pm_stride):
    """(stride, rec_pitch, msk_pitch) as the device entry points that read witness rows take them, from CUDA tensors: a pitch of 0 is taken from a string-major
    (B, M, D) / (B, M) view's strides.  records None: record planes; masked None: a reader without masked rows."""
    if chars_pm_stride is not None:
        stride = int(chars_pm_stride)
        assert layout & LAYOUT_INPUT_POSITION_MAJOR and chars.is_contiguous()
    else:
        assert not layout & LAYOUT_INPUT_POSITION_MAJOR and chars.stride(1) == 1
        stride = chars.stride(0)
    if not layout & LAYOUT_POSITION_MAJOR:
        if not rec_pitch and records is not None and records.dim() == 3:
            rec_pitch = records.stride(0) // D
        if not msk_pitch and masked is not None and masked.dim() == 2:
            msk_pitch = masked.stride(0)
    return stride, int(rec_pitch), int(msk_pitch)


def _theta_stride(theta, count, dtype):
    """theta_stride of the compress entry points for a contiguous (count, 4) — 4 — or (4,) — 0 — array or tensor of limbs"""
    shape = tuple(theta.shape)
    contiguous = theta.is_contiguous() if hasattr(theta, "is_contiguous") else theta.flags.c_contiguous
    if theta.dtype != dtype or not contiguous or shape not in ((4,), (count, 4)):
        raise HrxError(HRX_ERR_ARG, "theta: contiguous 64-bit limbs of shape (4,) or (%d, 4)" % count)
    return 0 if shape == (4,) else 4


def _out_buffer(buf, name, shape, dtype, device=None, zeros=False):
    """An output buffer of `shape` and `dtype` (a torch dtype: a tensor on `device`; otherwise a numpy array): the caller's `buf` if it has this dtype, is
    contiguous and holds exactly that many elements, else HrxError(HRX_ERR_ARG); buf None: a fresh one, uninitialised unless zeros (numpy only)."""
    on_torch = isinstance(dtype, torch.dtype)
    if buf is None:
        return torch.empty(shape, dtype=dtype, device=device) if on_torch else (np.zeros if zeros else np.empty)(shape, dtype)
    if buf.dtype != dtype or not (buf.is_contiguous() if on_torch else buf.flags.c_contiguous) or (buf.numel() if on_torch else buf.size) != int(np.prod(shape)):
        kind = "%s tensor" % str(dtype).replace("torch.", "") if on_torch else "%s array" % np.dtype(dtype).name
        raise HrxError(HRX_ERR_ARG, "%s: a contiguous %s of %s elements" % (name, kind, "".join("[%d]" % x for x in shape)))
    return buf


def _planes_array(planes):
    """the `const uint32_t *const *record_planes` argument of the _planes entry points out of a list of CUDA tensors"""
    return (C.c_void_p * len(planes))(*[p.data_ptr() for p in planes])


def _numpy_rows(chars, records, masked, layout, D, rec_pitch, msk_pitch, chars_pm_stride):
    """(chars, records, masked, stride, rec_pitch, msk_pitch) as the host entry points that read witness rows take them, from numpy arrays: the flat
    position-major buffers contiguous, a pitch of 0 taken from a string-major view's strides.  masked None: a reader without masked rows."""
    ch, rec = np.asarray(chars), np.asarray(records)
    msk = None if masked is None else np.asarray(masked)
    if layout & LAYOUT_POSITION_MAJOR:
        rec = np.ascontiguousarray(rec)
        msk = None if msk is None else np.ascontiguousarray(msk)
    else:
        if not rec_pitch and rec.ndim == 3:
            assert rec.strides[2] == 4 and rec.strides[1] == 4 * D
            rec_pitch = rec.strides[0] // (4 * D)
        if not msk_pitch and msk is not None and msk.ndim == 2:
            assert msk.strides[1] == 2
            msk_pitch = msk.strides[0] // 2
    if chars_pm_stride is not None:
        stride, ch = int(chars_pm_stride), np.ascontiguousarray(ch)
    else:
        assert ch.ndim == 2 and ch.strides[1] == 1
        stride = ch.strides[0]
    return ch, rec, msk, stride, int(rec_pitch), int(msk_pitch)


class RegexVerifyConfig:
    """Witness-side mirror of RegexVerifyConfig (src/lib.rs:96-113).

    configure() takes what the reference's configure (lib.rs:126-131) takes minus the halo2 objects
    (ConstraintSystem, FlexGateConfig): max_chars_size and the Vec<RegexDefs>.  `device=None` builds the
    host-side tables only (table rows, constants); any compute call then raises.  `device=HRX_DEVICE_NONE`
    makes a host-only context: match_substrs / derive_* / witness_batch_host run the library's native
    small-batch host walk (what a drop-in for the one-string-per-call lib.rs:316-318 needs), device batches raise.
    """

    def __init__(self, max_chars_size, regex_defs, device=0):
        self.max_chars_size = int(max_chars_size)
        self.regex_defs = list(regex_defs)      # pub field, lib.rs:112
        self._defs = _DefsHandle(self.regex_defs)
        self.num_defs = lib.hrx_defs_num_defs(self._defs.h)
        self.table_array = [RegexTableConfig(self._defs, d) for d in range(self.num_defs)]
        self._ctx = None
        self.device = device
        if device is not None:   # a GPU index, or HRX_DEVICE_NONE for the host-only context
            ctx = C.c_void_p()
            _check(lib.hrx_ctx_create(self._defs.h, int(device), C.byref(ctx)))
            self._ctx = ctx

    @classmethod
    def configure(cls, max_chars_size, regex_defs, device=0):
        return cls(max_chars_size, regex_defs, device)

    def __del__(self):
        if getattr(self, "_ctx", None) and lib is not None:
            lib.hrx_ctx_destroy(self._ctx)
            self._ctx = None

    def clone(self, device=HRX_DEVICE_SAME):
        """hrx_ctx_clone: RegexVerifyConfig derives Clone (lib.rs:96) — the same config with a context (stream, scratch, lock) of its own, e.g. one per prover thread."""
        import copy
        ctx = C.c_void_p()
        _check(lib.hrx_ctx_clone(self._need_ctx(), int(device), C.byref(ctx)))   # first: a failed clone must leave nothing behind that owns the source's context
        c = copy.copy(self)
        c._ctx = ctx
        c.device = self.device if device == HRX_DEVICE_SAME else device
        return c

    def _need_ctx(self):
        if not self._ctx:
            raise HrxError(HRX_ERR_HIP, "no context: configure(..., device=k) for a gfx950 GPU or device=HRX_DEVICE_NONE for the host walk")
        return self._ctx

    def _need_device(self, *tensors):
        """The batch kernels run on this config's device: every tensor must live there."""
        ctx = self._need_ctx()
        for t in tensors:
            if t is not None and (not t.is_cuda or t.device.index != self.device):
                raise HrxError(HRX_ERR_ARG, "tensor on %s but the config's context is on cuda:%s" % (t.device, self.device))
        return ctx

    def set_host_threshold(self, rows):
        """hrx_ctx_set_host_threshold: host-buffer batches of fewer than `rows` witness rows take the host walk."""
        _check(lib.hrx_ctx_set_host_threshold(self._need_ctx(), int(rows)))

    def host_threshold(self):
        return lib.hrx_ctx_host_threshold(self._need_ctx())

    def set_placement(self, walk=True, max_bytes=0, max_ms=0.0):
        """hrx_ctx_set_placement: placement-aware output allocation of this config's context off / on, and the memory / time budget of one walk (0 = default)."""
        _check(lib.hrx_ctx_set_placement(self._need_ctx(), PLACE_WALK if walk else PLACE_OFF, int(max_bytes), float(max_ms)))

    # -- lookup tables: RegexVerifyConfig::load (lib.rs:779-785) ---------------------------------
    def load(self):
        """Returns per def (transition_rows, endpoint_rows) in table.rs assignment order."""
        return [(t.transition_rows(), t.endpoint_rows()) for t in self.table_array]

    def substr_id_offset(self, d):
        return lib.hrx_defs_substr_id_offset(self._defs.h, d)

    def accepted_state(self, d):
        return lib.hrx_defs_accepted_state(self._defs.h, d)

    def first_state(self, d):
        return lib.hrx_defs_first_state(self._defs.h, d)

    def table_bytes(self):
        return lib.hrx_defs_table_bytes(self._defs.h)

    def describe_launch(self, B, layout=0, num_cus=256):
        """Kernel name and launch geometry the planner picks for B strings in `layout` (include/hrx.h: 0 string-major, 1 position-major
        outputs, 3 position-major input and outputs); host-only; MI355X has 256 CUs."""
        buf = C.create_string_buffer(4096)
        if self._ctx and num_cus == 256:    # the context's own view: its device's CUs, the flags it was created with, its set_option choices
            _check(lib.hrx_ctx_describe_launch(self._ctx, layout, B, self.max_chars_size, buf, 4096))
        else:
            _check(lib.hrx_describe_launch(self._defs.h, layout, B, self.max_chars_size, num_cus, buf, 4096))
        return buf.value.decode()

    # -- the three derive_* of lib.rs:804-888 -----------------------------------------------------
    def derive_states(self, characters):
        ch = np.frombuffer(bytes(characters), dtype=np.uint8)
        n = len(ch)
        states = np.zeros((self.num_defs, n + 1), np.uint64)
        _check(lib.hrx_derive_states(self._need_ctx(), _ptr(ch, _u8p) if n else None, n, _ptr(states, _u64p)))
        return states

    def derive_substr_ids(self, states):
        states = _np(states, np.uint64)
        n = states.shape[1] - 1
        out = np.zeros((self.num_defs, n), np.uint64)
        _check(lib.hrx_derive_substr_ids(self._need_ctx(), _ptr(states, _u64p), n, _ptr(out, _u64p)))
        return out

    def derive_is_start_end(self, states, substr_ids):
        states = _np(states, np.uint64)
        substr_ids = _np(substr_ids, np.uint64)
        n = states.shape[1] - 1
        st = np.zeros((self.num_defs, n + 1), np.uint8)
        en = np.zeros((self.num_defs, n + 1), np.uint8)
        _check(lib.hrx_derive_is_start_end(self._need_ctx(), _ptr(states, _u64p), _ptr(substr_ids, _u64p), n,
                                           _ptr(st, _u8p), _ptr(en, _u8p)))
        return st.astype(bool), en.astype(bool)

    # -- match_substrs (lib.rs:311-773), integer columns ------------------------------------------
    def match_substrs(self, characters):
        ch = np.frombuffer(bytes(characters), dtype=np.uint8)
        n, M, D = len(ch), self.max_chars_size, self.num_defs
        cols = {k: np.zeros(M, np.uint64) for k in ("enable", "character", "masked_char", "masked_substr_id")}
        for k in ("state", "substr_id", "start_enable", "end_enable"):
            cols[k] = np.zeros((D, M), np.uint64)
        status = np.zeros(1, np.uint64)
        _check(lib.hrx_match_substrs(self._need_ctx(), _ptr(ch, _u8p) if n else None, n, M,
                                     *[_ptr(cols[k], _u64p) for k in ("enable", "character", "state", "substr_id",
                                                                       "start_enable", "end_enable", "masked_char",
                                                                       "masked_substr_id")], _ptr(status, _u64p)))
        return AssignedRegexResult(all_enable_flags=cols["enable"], all_characters=cols["character"],
                                   all_substr_ids=cols["masked_substr_id"], masked_characters=cols["masked_char"],
                                   states=cols["state"], substr_ids=cols["substr_id"],
                                   start_enables=cols["start_enable"], end_enables=cols["end_enable"],
                                   status=int(status[0]))

    # -- the batch surface (the build's addition; parity is per string with match_substrs) --------
    def witness_batch_host(self, chars2d, lens, out=None):
        """chars2d (B, stride) uint8 numpy, lens (B,) -> records (B,M,D) u32, masked (B,M) u16, status (B,) u64.
        out=(rec, msk, st): reuse the caller's arrays (fresh arrays cost a page fault per 4 KiB while the copy lands)."""
        chars2d = _np(chars2d, np.uint8)
        lens = _np(lens, np.uint32)
        B, stride = chars2d.shape
        M, D = self.max_chars_size, self.num_defs
        if out is None:
            out = np.zeros((B, M, D), np.uint32), np.zeros((B, M), np.uint16), np.zeros(B, np.uint64)
        rec, msk, st = out
        assert rec.shape == (B, M, D) and msk.shape == (B, M) and st.shape == (B,) and rec.flags.c_contiguous and msk.flags.c_contiguous
        _check(lib.hrx_witness_batch_host(self._need_ctx(), _ptr(chars2d, _u8p), stride, _ptr(lens, _u32p), B, M,
                                          _ptr(rec, _u32p), _ptr(msk, _u16p), _ptr(st, _u64p)))
        return rec, msk, st

    # -- match only: status + revealed spans, no witness rows (include/hrx.h MATCH) ----------------
    def match_batch_host(self, chars2d, lens, max_spans=16):
        """chars2d (B, stride) uint8 numpy, lens (B,) -> status (B,) u64, counts (B,) u32, spans (B, max_spans) u64 (decode_spans)."""
        chars2d = _np(chars2d, np.uint8)
        lens = _np(lens, np.uint32)
        B, stride = chars2d.shape
        st = np.zeros(B, np.uint64)
        cnt = np.zeros(B, np.uint32)
        sp = np.zeros((B, max_spans), np.uint64)
        _check(lib.hrx_match_batch_host(self._need_ctx(), _ptr(chars2d, _u8p), stride, _ptr(lens, _u32p), B, self.max_chars_size,
                                        _ptr(st, _u64p), _ptr(cnt, _u32p), _ptr(sp, _u64p) if max_spans else None, max_spans))
        return st, cnt, sp

    def match_batch(self, chars, lens, max_spans=16, stream=None, chars_pm_stride=None, out=None):
        """Device-resident batch (as witness_batch; chars_pm_stride: the position-major input of chars_to_position_major) ->
        (status (B,) int64, counts (B,) int32, spans (B, max_spans) int64) CUDA tensors holding the u64 / u32 / u64 words of include/hrx.h.
        Asynchronous on `stream` (default: torch's current stream).  out=(status, counts, spans): the caller's tensors."""
        assert chars.is_cuda and lens.is_cuda and chars.dtype == torch.uint8 and lens.dtype == torch.int32 and lens.is_contiguous()
        if chars_pm_stride is None:
            assert chars.stride(1) == 1
            B, stride, layout = chars.shape[0], chars.stride(0), LAYOUT_STRING_MAJOR
        else:
            assert chars.is_contiguous() and chars.numel() == lens.numel() * chars_pm_stride
            B, stride, layout = lens.numel(), int(chars_pm_stride), LAYOUT_INPUT_POSITION_MAJOR
        if out is None:
            out = (torch.empty(B, dtype=torch.int64, device=chars.device), torch.empty(B, dtype=torch.int32, device=chars.device),
                   torch.empty((B, max(max_spans, 1)), dtype=torch.int64, device=chars.device))
        st, cnt, sp = out
        s = torch.cuda.current_stream(chars.device) if stream is None else stream
        _check(lib.hrx_match_batch_device(self._need_device(chars, lens, st, cnt, sp), layout, chars.data_ptr(), stride, lens.data_ptr(), B,
                                          self.max_chars_size, st.data_ptr(), cnt.data_ptr(), sp.data_ptr() if max_spans else None, max_spans,
                                          s.cuda_stream))
        return st, cnt, sp

    # -- ragged input: values + offsets, no padding (include/hrx.h RAGGED) ----------------------------------------------
    def match_batch_host_ragged(self, values, offsets, max_spans=16):
        """values (uint8) + offsets (B + 1, uint64) host arrays (pack_strings), string b = values[offsets[b]:offsets[b + 1]] ->
        status (B,) u64, counts (B,) u32, spans (B, max_spans) u64, bit for bit what match_batch_host gives the padded batch."""
        values = _np(values, np.uint8)
        offsets = _np(offsets, np.uint64)
        B = len(offsets) - 1
        assert B >= 0
        st = np.zeros(B, np.uint64)
        cnt = np.zeros(B, np.uint32)
        sp = np.zeros((B, max_spans), np.uint64)
        vals = values if values.size else np.zeros(16, np.uint8)
        _check(lib.hrx_match_batch_host_ragged(self._need_ctx(), _ptr(vals, _u8p), _ptr(offsets, _u64p) if B else None, B, self.max_chars_size,
                                               _ptr(st, _u64p), _ptr(cnt, _u32p), _ptr(sp, _u64p) if max_spans else None, max_spans))
        return st, cnt, sp

    def match_strings(self, strings, max_spans=16):
        """A list of bytes on the host (match_batch_host_ragged of pack_strings(strings)) -> (status, counts, spans)."""
        return self.match_batch_host_ragged(*pack_strings(strings), max_spans=max_spans)

    def match_batch_ragged(self, values, offsets, max_spans=16, stream=None, out=None):
        """Device-resident ragged batch: values uint8 CUDA tensor (16-byte aligned; readable up to the 16-byte chunk end of every string's last
        byte, as pack_strings pads it), offsets int64 CUDA tensor of B + 1 entries -> the tensors match_batch returns.  Asynchronous on
        `stream` (default: torch's current stream).  out=(status, counts, spans): the caller's tensors."""
        assert values.is_cuda and offsets.is_cuda and values.dtype == torch.uint8 and offsets.dtype == torch.int64
        assert values.is_contiguous() and offsets.is_contiguous() and offsets.dim() == 1
        B = offsets.numel() - 1
        if out is None:
            out = (torch.empty(B, dtype=torch.int64, device=values.device), torch.empty(B, dtype=torch.int32, device=values.device),
                   torch.empty((B, max(max_spans, 1)), dtype=torch.int64, device=values.device))
        st, cnt, sp = out
        s = torch.cuda.current_stream(values.device) if stream is None else stream
        _check(lib.hrx_match_batch_device_ragged(self._need_device(values, offsets, st, cnt, sp), values.data_ptr(), offsets.data_ptr(), B,
                                                 self.max_chars_size, st.data_ptr(), cnt.data_ptr(), sp.data_ptr() if max_spans else None, max_spans,
                                                 s.cuda_stream))
        return st, cnt, sp

    def ragged_to_position_major(self, values, offsets, stride=None, out=None, stream=None):
        """hrx_ragged_to_position_major_device: a device-resident ragged batch -> (chars_pm, lens): the flat HRX_LAYOUT_INPUT_POSITION_MAJOR buffer
        with per-string capacity `stride` (default: max_chars_size rounded up to 16) and lens int32 (-1 = UINT32_MAX: longer than stride or
        decreasing offsets), the input of witness_batch_position_major / witness_batch_planes / match_batch with chars_pm_stride=stride."""
        assert values.is_cuda and offsets.is_cuda and values.dtype == torch.uint8 and offsets.dtype == torch.int64 and offsets.is_contiguous()
        B = offsets.numel() - 1
        stride = -(-self.max_chars_size // 16) * 16 if stride is None else int(stride)
        if out is None:
            out = (torch.empty((B * stride,), dtype=torch.uint8, device=values.device), torch.empty(B, dtype=torch.int32, device=values.device))
        chars_pm, lens = out
        s = torch.cuda.current_stream(values.device) if stream is None else stream
        _check(lib.hrx_ragged_to_position_major_device(self._need_device(values, offsets, chars_pm, lens), values.data_ptr(), offsets.data_ptr(), B,
                                                       stride, chars_pm.data_ptr(), lens.data_ptr(), s.cuda_stream))
        return chars_pm, lens

    # -- extract: the revealed bytes as a list column (include/hrx.h EXTRACT) ------------------------------------------------
    def alloc_extract(self, B, max_spans, values_cap, runs_cap=None, device=None):
        """Device tensors for extract_spans / extract_batch*: (status, counts, spans, run_offsets, runs, byte_offsets, values, totals, workspace);
        runs_cap defaults to B * max_spans, which always suffices, as values_cap = the input's byte count does."""
        dev = torch.device("cuda", self.device) if device is None else torch.device(device)
        runs_cap = B * max_spans if runs_cap is None else int(runs_cap)
        i64 = lambda n: torch.empty(int(n), dtype=torch.int64, device=dev)
        return (i64(B), torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, max_spans), dtype=torch.int64, device=dev), i64(B + 1), i64(runs_cap),
                i64(runs_cap + 1), torch.empty(int(values_cap), dtype=torch.uint8, device=dev), i64(4), i64(extract_workspace_bytes(B) // 8))

    def extract_spans(self, src, status, counts, spans, out, offsets=None, chars_pm_stride=None, require_accept=0, stream=None):
        """hrx_extract_spans_device on the outputs of a match call: src = chars (B, stride), the position-major buffer (chars_pm_stride) or ragged values
        (offsets); out = the tensors of alloc_extract from run_offsets on (run_offsets, runs, byte_offsets, values, totals, workspace): the caps are their
        sizes.  Asynchronous on `stream`; four launches, nothing allocated."""
        ro, runs, bo, vals, tot, ws = out
        B, max_spans = status.numel(), spans.shape[1]
        if offsets is not None:
            layout, stride = LAYOUT_INPUT_RAGGED, 0
        elif chars_pm_stride is not None:
            layout, stride = LAYOUT_INPUT_POSITION_MAJOR, int(chars_pm_stride)
        else:
            assert src.stride(1) == 1
            layout, stride = LAYOUT_STRING_MAJOR, src.stride(0)
        assert ro.numel() == B + 1 and bo.numel() == runs.numel() + 1 and tot.numel() == 4 and spans.is_contiguous()
        o = _ExtractOutC(ro.data_ptr(), runs.data_ptr(), bo.data_ptr(), vals.data_ptr(), tot.data_ptr(), runs.numel(), vals.numel())
        s = torch.cuda.current_stream(status.device) if stream is None else stream
        _check(lib.hrx_extract_spans_device(self._need_device(src, offsets, status, counts, spans, ro, runs, bo, vals, tot, ws), layout, src.data_ptr(), stride,
                                            offsets.data_ptr() if offsets is not None else None, B, status.data_ptr(), counts.data_ptr(), spans.data_ptr(), max_spans,
                                            int(require_accept), C.byref(o), ws.data_ptr(), ws.numel() * 8, s.cuda_stream))
        return Extracted(status, counts, ro, runs, bo, vals, tot)

    def extract_batch(self, chars, lens, max_spans=16, chars_pm_stride=None, require_accept=0, caps=None, stream=None, out=None):
        """match_batch + extract_spans on one stream: a device-resident batch -> Extracted(status, counts, run_offsets, runs, byte_offsets, values, totals),
        CUDA tensors holding the words of include/hrx.h EXTRACT.  caps = (runs_cap, values_cap), default the always-sufficient B * max_spans and the input's
        byte count; out: the nine tensors of alloc_extract (its sizes are the caps then).  Nothing but the revealed bytes has to leave the device:
        totals says how much of runs / byte_offsets / values is filled."""
        B = lens.numel()
        if out is None:
            caps = caps or (B * max_spans, chars.numel())
            out = self.alloc_extract(B, max_spans, caps[1], caps[0], chars.device)
        st, cnt, sp = self.match_batch(chars, lens, max_spans=max_spans, stream=stream, chars_pm_stride=chars_pm_stride, out=out[:3])
        return self.extract_spans(chars, st, cnt, sp, out[3:], chars_pm_stride=chars_pm_stride, require_accept=require_accept, stream=stream)

    def extract_batch_ragged(self, values, offsets, max_spans=16, require_accept=0, caps=None, stream=None, out=None):
        """extract_batch for a device-resident ragged batch (match_batch_ragged + extract_spans): a column in, a column out."""
        B = offsets.numel() - 1
        if out is None:
            caps = caps or (B * max_spans, values.numel())
            out = self.alloc_extract(B, max_spans, caps[1], caps[0], values.device)
        st, cnt, sp = self.match_batch_ragged(values, offsets, max_spans=max_spans, stream=stream, out=out[:3])
        return self.extract_spans(values, st, cnt, sp, out[3:], offsets=offsets, require_accept=require_accept, stream=stream)

    def extract_batch_host(self, chars2d, lens, max_spans=16, require_accept=0, caps=None, out=None):
        """Host arrays in, host arrays out, on either kind of context: match_batch_host, then hrx_extract_spans_host on the bytes where they are."""
        chars2d = _np(chars2d, np.uint8)
        st, cnt, sp = self.match_batch_host(chars2d, lens, max_spans=max_spans)
        return extract_spans_host(chars2d, st, cnt, sp, require_accept=require_accept, caps=caps, out=out)

    def extract_batch_host_ragged(self, values, offsets, max_spans=16, require_accept=0, caps=None, out=None):
        values, offsets = _np(values, np.uint8), _np(offsets, np.uint64)
        st, cnt, sp = self.match_batch_host_ragged(values, offsets, max_spans=max_spans)
        return extract_spans_host(values, st, cnt, sp, offsets=offsets, require_accept=require_accept, caps=caps, out=out)

    def extract_strings(self, strings, max_spans=16, require_accept=0):
        """A list of bytes on the host -> Extracted (extract_batch_host_ragged of pack_strings(strings)); extracted_lists gives it per string."""
        return self.extract_batch_host_ragged(*pack_strings(strings), max_spans=max_spans, require_accept=require_accept)

    # -- route: the screened batch by circuit-size bucket, each bucket staged for the witness (include/hrx.h ROUTE) --------------
    def route(self, status, lens=None, offsets=None, bounds=None, require_accept=0, stream=None, out=None):
        """hrx_route_device: status (B,) int64 of a match call (or None: no screening) and the strings' lengths — lens (B,) int32 or ragged offsets
        (B + 1,) int64, exactly one of them — -> Routed(order (B,) int32, bucket_offsets (n_buckets + 2,) int64): bucket j (strings that pass the screen
        with n <= bounds[j], and > bounds[j - 1]) is order[bucket_offsets[j]:bucket_offsets[j + 1]], range n_buckets the strings that were not kept, every
        range in increasing b.  bounds: a host list of at most MAX_BUCKETS circuit sizes, default [max_chars_size].  Asynchronous on `stream`; three
        launches, nothing allocated when out=(order, bucket_offsets, workspace int64 of route_workspace_bytes(B) // 8 words) is given."""
        bounds = _np([self.max_chars_size] if bounds is None else bounds, np.uint32)
        src = lens if lens is not None else offsets
        if src is None or (lens is not None and offsets is not None):
            raise HrxError(HRX_ERR_ARG, "route: exactly one of lens and offsets")
        B = lens.numel() if lens is not None else offsets.numel() - 1
        assert src.is_cuda and src.is_contiguous() and src.dtype == (torch.int32 if lens is not None else torch.int64)
        assert status is None or (status.dtype == torch.int64 and status.is_contiguous() and status.numel() == B)
        if out is None:
            out = (torch.empty(B, dtype=torch.int32, device=src.device), torch.empty(len(bounds) + 2, dtype=torch.int64, device=src.device),
                   torch.empty(route_workspace_bytes(B) // 8, dtype=torch.int64, device=src.device))
        order, bo, ws = out
        assert order.numel() == B and bo.numel() == len(bounds) + 2 and order.dtype == torch.int32 and bo.dtype == torch.int64
        s = torch.cuda.current_stream(src.device) if stream is None else stream
        # (an empty tensor has no address, and the C rule names the form by its non-NULL pointer: nothing is read at B = 0, any device address does)
        at = lambda t: None if t is None else (t.data_ptr() or bo.data_ptr())
        _check(lib.hrx_route_device(self._need_device(status, src, order, bo, ws), status.data_ptr() if status is not None else None, int(require_accept),
                                    at(lens), at(offsets), B,
                                    _ptr(bounds, _u32p), len(bounds), order.data_ptr(), bo.data_ptr(), ws.data_ptr(), ws.numel() * 8, s.cuda_stream))
        return Routed(order, bo)

    def gather_to_position_major(self, src, sel, stride, lens=None, offsets=None, out=None, stream=None):
        """hrx_gather_to_position_major_device: the strings sel (int32 CUDA tensor of string indices, e.g. order[bucket_offsets[j]:bucket_offsets[j + 1]])
        of a string-major batch (src (B, src_stride) uint8 with lens (B,) int32) or a ragged one (src = values with offsets (B + 1,) int64) ->
        (chars_pm, lens_out): the flat HRX_LAYOUT_INPUT_POSITION_MAJOR buffer of len(sel) slots of `stride` bytes and lens_out int32 (-1 = UINT32_MAX: an
        index past the batch, or a string that does not fit), the input of witness_batch_position_major / match_batch with chars_pm_stride=stride."""
        assert src.is_cuda and sel.is_cuda and src.dtype == torch.uint8 and sel.dtype == torch.int32 and sel.is_contiguous() and sel.dim() == 1
        if (lens is None) == (offsets is None):
            raise HrxError(HRX_ERR_ARG, "gather_to_position_major: exactly one of lens and offsets")
        if offsets is not None:
            assert offsets.dtype == torch.int64 and offsets.is_contiguous() and src.is_contiguous()
            layout, B, src_stride = LAYOUT_INPUT_RAGGED, offsets.numel() - 1, 0
        else:
            assert lens.dtype == torch.int32 and lens.is_contiguous() and src.dim() == 2 and src.stride(1) == 1
            layout, B, src_stride = LAYOUT_STRING_MAJOR, lens.numel(), src.stride(0)
        n_sel, stride = sel.numel(), int(stride)
        if out is None:
            out = (torch.empty((n_sel * stride,), dtype=torch.uint8, device=src.device), torch.empty(n_sel, dtype=torch.int32, device=src.device))
        chars_pm, lens_out = out
        assert chars_pm.numel() == n_sel * stride and lens_out.numel() == n_sel
        s = torch.cuda.current_stream(src.device) if stream is None else stream
        _check(lib.hrx_gather_to_position_major_device(self._need_device(src, sel, lens, offsets, chars_pm, lens_out), layout, src.data_ptr(), src_stride,
                                                       lens.data_ptr() if lens is not None else None, offsets.data_ptr() if offsets is not None else None,
                                                       B, sel.data_ptr(), n_sel, stride, chars_pm.data_ptr(), lens_out.data_ptr(), s.cuda_stream))
        return chars_pm, lens_out

    # -- selected: the match of a selection of a batch, in its order (include/hrx.h SELECTED) ------------------------------------
    def match_selected(self, src, sel, lens=None, offsets=None, max_spans=16, stream=None, out=None):
        """hrx_match_selected_device: the match of the strings sel (int32 CUDA tensor of string indices, as route returns them in order) of a string-major
        batch (src (B, src_stride) uint8 with lens (B,) int32) or a ragged one (src = values with offsets (B + 1,) int64), walked in sel's order ->
        (status (B,), counts (B,), spans (B, max_spans)) indexed by STRING as match_batch / match_batch_ragged return them: the entries of the strings
        in sel are what those calls give, every other entry is left as it was (out=(status, counts, spans): the caller's pre-filled tensors; without
        out the tensors are fresh and unselected entries hold nothing meaningful).  An index >= B is skipped.  Asynchronous on `stream`."""
        assert src.is_cuda and sel.is_cuda and src.dtype == torch.uint8 and sel.dtype == torch.int32 and sel.is_contiguous() and sel.dim() == 1
        if (lens is None) == (offsets is None):
            raise HrxError(HRX_ERR_ARG, "match_selected: exactly one of lens and offsets")
        if offsets is not None:
            assert offsets.dtype == torch.int64 and offsets.is_contiguous() and src.is_contiguous()
            layout, B, src_stride = LAYOUT_INPUT_RAGGED, offsets.numel() - 1, 0
        else:
            assert lens.dtype == torch.int32 and lens.is_contiguous() and src.dim() == 2 and src.stride(1) == 1
            layout, B, src_stride = LAYOUT_STRING_MAJOR, lens.numel(), src.stride(0)
        if out is None:
            out = (torch.empty(B, dtype=torch.int64, device=src.device), torch.empty(B, dtype=torch.int32, device=src.device),
                   torch.empty((B, max(max_spans, 1)), dtype=torch.int64, device=src.device))
        st, cnt, sp = out
        assert st.numel() == B and cnt.numel() == B and sp.shape[0] == B and sp.is_contiguous()
        s = torch.cuda.current_stream(src.device) if stream is None else stream
        _check(lib.hrx_match_selected_device(self._need_device(src, sel, lens, offsets, st, cnt, sp), layout, src.data_ptr(), src_stride,
                                             lens.data_ptr() if lens is not None else None, offsets.data_ptr() if offsets is not None else None, B,
                                             sel.data_ptr() if sel.numel() else None, sel.numel(), self.max_chars_size, st.data_ptr(), cnt.data_ptr(),
                                             sp.data_ptr() if max_spans else None, max_spans, s.cuda_stream))
        return st, cnt, sp

    def match_selected_host(self, src, sel, lens=None, offsets=None, max_spans=16, out=None):
        """hrx_match_selected_host: host arrays — src (B, stride) uint8 with lens (B,), or src = values with offsets (B + 1,) uint64 — and sel (uint32
        string indices) -> (status (B,) u64, counts (B,) u32, spans (B, max_spans) u64) indexed by string; entries of strings not in sel keep what
        out=(status, counts, spans) held (fresh arrays: zero)."""
        if (lens is None) == (offsets is None):
            raise HrxError(HRX_ERR_ARG, "match_selected_host: exactly one of lens and offsets")
        src = _np(src, np.uint8)
        sel = _np(sel, np.uint32)
        if offsets is not None:
            offsets = _np(offsets, np.uint64)
            layout, B, stride = LAYOUT_INPUT_RAGGED, len(offsets) - 1, 0
            if not src.size:
                src = np.zeros(16, np.uint8)
        else:
            lens = _np(lens, np.uint32)
            layout, (B, stride) = LAYOUT_STRING_MAJOR, src.shape
        if out is None:
            out = np.zeros(B, np.uint64), np.zeros(B, np.uint32), np.zeros((B, max_spans), np.uint64)
        st, cnt, sp = out
        assert st.shape == (B,) and cnt.shape == (B,) and sp.shape == (B, max_spans) and st.dtype == np.uint64 and cnt.dtype == np.uint32 and sp.dtype == np.uint64
        assert sp.flags.c_contiguous
        _check(lib.hrx_match_selected_host(self._need_ctx(), layout, src.ctypes.data, stride, lens.ctypes.data if lens is not None else None,
                                           offsets.ctypes.data if offsets is not None else None, B, sel.ctypes.data if sel.size else None, sel.size,
                                           self.max_chars_size, st.ctypes.data, cnt.ctypes.data, sp.ctypes.data if max_spans else None, max_spans))
        return st, cnt, sp

    @contextlib.contextmanager
    def circuit_size(self, M):
        """`with cfg.circuit_size(M):` — this config's calls at another max_chars_size.  M is a per-call argument of every entry point of include/hrx.h, so
        one context serves every circuit size a router sorts strings into."""
        old, self.max_chars_size = self.max_chars_size, int(M)
        try:
            yield self
        finally:
            self.max_chars_size = old

    def describe_match(self, B, layout=0, num_cus=256):
        """hrx_ctx_describe_match (or hrx_describe_match without a context): the kernel(s) match_batch runs for B strings, as text."""
        buf = C.create_string_buffer(4096)
        if self._ctx:
            _check(lib.hrx_ctx_describe_match(self._ctx, layout, B, self.max_chars_size, buf, 4096))
        else:
            _check(lib.hrx_describe_match(self._defs.h, layout, B, self.max_chars_size, num_cus, buf, 4096))
        return buf.value.decode()

    def alloc_outputs(self, B, device=None, pitched=False):
        """Device buffers for witness_batch: records int32 (B,M,D), masked int16 (B,M), status int64 (B,).
        pitched=True: the same shapes as views into buffers whose per-string pitch is hrx_recommended_pitches(M)
        (rows M.. of each string's slot are never written)."""
        dev = torch.device("cuda", self.device) if device is None else device
        M, D = self.max_chars_size, self.num_defs
        rp, mp = (recommended_pitches(M)[:2] if pitched else (M, M))
        st = torch.empty((B,), dtype=torch.int64, device=dev)
        if B * rp * D * 4 >= PLACED_FROM and dev.index in (None, self.device) and not torch.cuda.is_current_stream_capturing():     # several GB: a pair that does not collide
            pr, pmk = C.c_void_p(), C.c_void_p()
            _check(lib.hrx_alloc_output_pair(self._ctx, B * rp * D * 4, B * mp * 2, C.byref(pr), C.byref(pmk)))
            d = torch.device("cuda", self.device)
            rec = torch.as_tensor(_LibraryOwned(pr.value, B * rp * D * 4), device=d).view(torch.int32).view(B, rp, D)[:, :M]
            msk = torch.as_tensor(_LibraryOwned(pmk.value, B * mp * 2), device=d).view(torch.int16).view(B, mp)[:, :M]
            return rec, msk, st
        rec = torch.empty((B, rp, D), dtype=torch.int32, device=dev)[:, :M]
        msk = torch.empty((B, mp), dtype=torch.int16, device=dev)[:, :M]
        return rec, msk, st

    def alloc_outputs_position_major(self, B, device=None):
        """Flat device buffers for HRX_LAYOUT_POSITION_MAJOR: records int32 [ceil(M/4)*B*4*D], masked int16 [ceil(M/8)*B*8].
        (The status tensor — and, below the placement threshold, all three — comes from torch's caching allocator on the CURRENT stream: launch on that stream, or order
        the launch stream behind it, as with any torch tensor used on a side stream.)"""
        dev = torch.device("cuda", self.device) if device is None else device
        nr, nm = C.c_size_t(0), C.c_size_t(0)
        lib.hrx_position_major_sizes(B, self.max_chars_size, self.num_defs, C.byref(nr), C.byref(nm))
        st = torch.empty((B,), dtype=torch.int64, device=dev)
        if nr.value * 4 < PLACED_FROM or dev.index not in (None, self.device) or torch.cuda.is_current_stream_capturing():     # (the search allocates and measures: not inside a stream capture)
            return torch.empty((nr.value,), dtype=torch.int32, device=dev), torch.empty((nm.value,), dtype=torch.int16, device=dev), st
        # several GB: the library allocates the pair and keeps the masked-row buffer that does not collide with the records
        pr, pmk = C.c_void_p(), C.c_void_p()
        _check(lib.hrx_alloc_outputs_position_major(self._ctx, B, self.max_chars_size, C.byref(pr), C.byref(pmk)))
        d = torch.device("cuda", self.device)
        rec = torch.as_tensor(_LibraryOwned(pr.value, nr.value * 4), device=d).view(torch.int32)
        msk = torch.as_tensor(_LibraryOwned(pmk.value, nm.value * 2), device=d).view(torch.int16)
        return rec, msk, st

    def alloc_output_planes(self, B, device=None, stripes=None, chars=None, lens=None, chars_pm_stride=None):
        """hrx_alloc_output_planes: ([record buffers] int32, masked int16, status int64) — every def's records in a buffer of its own (one def: the ordinary records buffer, or with
        stripes=2 its two row stripes), each placed in a neighbourhood of the device memory of its own (include/hrx.h: the launch's write streams spread over the classes of the
        physical address space).  chars / lens (as witness_batch_planes takes them): hrx_alloc_output_planes_for_batch — the launches that choose among the candidate sets run this
        batch, not a stand-in."""
        dev = torch.device("cuda", self.device) if device is None else device
        D = self.num_defs
        R = 1 if stripes is None else int(stripes)
        assert R == 1 or D == 1
        n = D * R
        npl, nm = C.c_size_t(0), C.c_size_t(0)
        lib.hrx_position_major_stripe_sizes(B, self.max_chars_size, R, C.byref(npl), C.byref(nm))
        st = torch.empty((B,), dtype=torch.int64, device=dev)
        if npl.value * 4 * n < PLACED_FROM or dev.index not in (None, self.device) or torch.cuda.is_current_stream_capturing():
            return [torch.empty((npl.value,), dtype=torch.int32, device=dev) for _ in range(n)], torch.empty((nm.value,), dtype=torch.int16, device=dev), st
        # (one def, one buffer: the library's pool of record AND masked-row candidates + a dry launch from 1 GiB of records on, its measured arena pair below)
        arr, pmk = (C.c_void_p * n)(), C.c_void_p()
        if chars is not None:
            assert lens is not None and chars.is_cuda and lens.is_cuda and chars.dtype == torch.uint8 and lens.dtype == torch.int32 and lens.numel() == B
            layout = LAYOUT_POSITION_MAJOR
            if chars_pm_stride is None:
                assert chars.stride(1) == 1 and lens.is_contiguous() and chars.shape[0] == B
                stride = chars.stride(0)
            else:
                assert chars.is_contiguous() and chars.numel() == B * chars_pm_stride
                stride = int(chars_pm_stride)
                layout |= LAYOUT_INPUT_POSITION_MAJOR
            torch.cuda.current_stream(chars.device).synchronize()       # (the library's launches run on the context's stream)
            _check(lib.hrx_alloc_output_planes_for_batch(self._need_device(chars, lens), layout, chars.data_ptr(), stride, lens.data_ptr(), B, self.max_chars_size, n, arr, C.byref(pmk)))
        else:
            _check(lib.hrx_alloc_output_planes(self._ctx, B, self.max_chars_size, n, arr, C.byref(pmk)))
        d = torch.device("cuda", self.device)
        planes = [torch.as_tensor(_LibraryOwned(arr[k], npl.value * 4), device=d).view(torch.int32) for k in range(n)]
        msk = torch.as_tensor(_LibraryOwned(pmk.value, nm.value * 2), device=d).view(torch.int16)
        return planes, msk, st

    def witness_batch_planes(self, chars, lens, out=None, stream=None, chars_pm_stride=None):
        """hrx_witness_batch_device_planes: like witness_batch_position_major with the record planes in D buffers (out = (planes, masked, status) as alloc_output_planes gives them)."""
        assert chars.is_cuda and lens.is_cuda and chars.dtype == torch.uint8 and lens.dtype == torch.int32
        layout = LAYOUT_POSITION_MAJOR
        if chars_pm_stride is None:
            assert chars.stride(1) == 1 and lens.is_contiguous()
            B, stride = chars.shape[0], chars.stride(0)
        else:
            assert chars.is_contiguous() and chars.numel() == lens.numel() * chars_pm_stride
            B, stride = lens.numel(), int(chars_pm_stride)
            layout |= LAYOUT_INPUT_POSITION_MAJOR
        if out is None:
            out = self.alloc_output_planes(B, chars.device)
        planes, msk, st = out
        arr = (C.c_void_p * len(planes))(*[p.data_ptr() for p in planes])
        s = torch.cuda.current_stream(chars.device) if stream is None else stream
        _check(lib.hrx_witness_batch_device_planes(self._need_device(chars, lens, msk, st, *planes), layout, chars.data_ptr(), stride, lens.data_ptr(), B, self.max_chars_size,
                                                   arr, len(planes), msk.data_ptr(), st.data_ptr(), s.cuda_stream))
        return planes, msk, st

    def traffic_pass_planes(self, chars_pm, B, out, chars_pm_stride, stream=None):
        """hrx_traffic_pass_device_planes: the memory traffic of one record-planes launch over these buffers, no DFA work; OVERWRITES out."""
        planes, msk, _ = out
        arr = (C.c_void_p * len(planes))(*[p.data_ptr() for p in planes])
        s = torch.cuda.current_stream(chars_pm.device) if stream is None else stream
        _check(lib.hrx_traffic_pass_device_planes(self._need_device(chars_pm, msk, *planes), chars_pm.data_ptr(), int(chars_pm_stride), int(B), self.max_chars_size,
                                                  arr, len(planes), msk.data_ptr(), s.cuda_stream))

    def probe_write_pair(self, a, b, nbytes=None):
        """hrx_probe_write_pair: GB/s of two equal write streams over device tensors a and b (OVERWRITTEN): do they lie in colliding neighbourhoods of the device memory?"""
        nbytes = min(a.numel() * a.element_size(), b.numel() * b.element_size()) if nbytes is None else nbytes
        g = C.c_double(0.0)
        _check(lib.hrx_probe_write_pair(self._need_device(a, b), a.data_ptr(), b.data_ptr(), int(nbytes), C.byref(g)))
        return g.value

    def host_route_report(self):
        """hrx_ctx_host_route_report: what this config's last witness_batch_host call did (a dict)."""
        r = _HostRouteReportC()
        _check(lib.hrx_ctx_host_route_report(self._need_ctx(), C.byref(r), C.sizeof(r)))
        return {k: getattr(r, k) for k, _ in _HostRouteReportC._fields_}

    def set_option(self, option, value):
        """hrx_ctx_set_option (include/hrx.h HRX_OPT_*)."""
        _check(lib.hrx_ctx_set_option(self._need_ctx(), int(option), int(value)))

    def get_option(self, option):
        return lib.hrx_ctx_get_option(self._need_ctx(), int(option))

    def last_placement_report(self):
        """hrx_alloc_last_report: what the last placement-aware allocation of this config's context did (a dict)."""
        r = _PlaceReportC()
        _check(lib.hrx_alloc_last_report_sized(self._need_ctx(), C.byref(r), C.sizeof(r)))
        return {k: getattr(r, k) for k, _ in _PlaceReportC._fields_}

    def traffic_pass(self, chars_pm, B, out, chars_pm_stride, stream=None):
        """hrx_traffic_pass_device: the memory traffic of one position-major launch over these buffers, no DFA work; OVERWRITES out."""
        rec, msk, _ = out
        s = torch.cuda.current_stream(chars_pm.device) if stream is None else stream
        _check(lib.hrx_traffic_pass_device(self._need_device(chars_pm, rec, msk), chars_pm.data_ptr(), int(chars_pm_stride), int(B), self.max_chars_size,
                                           rec.data_ptr(), msk.data_ptr(), s.cuda_stream))

    def traffic_pass_string_major(self, chars, out, stream=None):
        """hrx_traffic_pass_device_layout(HRX_LAYOUT_STRING_MAJOR): the memory traffic of one string-major launch over these buffers (chars (B, stride) uint8;
        out = (records (B, M, D) view, masked (B, M) view, status) as alloc_outputs gives them, pitched or not), no DFA work; OVERWRITES out."""
        rec, msk, _ = out
        B, stride = chars.shape
        D = self.num_defs
        s = torch.cuda.current_stream(chars.device) if stream is None else stream
        _check(lib.hrx_traffic_pass_device_layout(self._need_device(chars, rec, msk), 0, chars.data_ptr(), int(stride), int(B), self.max_chars_size,
                                                  rec.data_ptr(), rec.stride(0) // D, msk.data_ptr(), msk.stride(0), s.cuda_stream))

    def chars_to_position_major_device(self, chars, out=None, stream=None):
        """hrx_chars_to_position_major_device: (B, stride) string-major bytes on the device (stride % 16 == 0, one contiguous string per row: the reference's
        input shape, lib.rs:311-315) -> the flat HRX_LAYOUT_INPUT_POSITION_MAJOR buffer (the library's own kernel; chars_to_position_major above does
        the same with torch ops).  Asynchronous on `stream` (default: torch's current stream)."""
        B, stride = chars.shape
        if not chars.is_contiguous():
            chars = chars.contiguous()
        if out is None:
            out = torch.empty((B * stride,), dtype=torch.uint8, device=chars.device)
        s = torch.cuda.current_stream(chars.device) if stream is None else stream
        _check(lib.hrx_chars_to_position_major_device(self._need_device(chars, out), chars.data_ptr(), int(stride), int(B), out.data_ptr(), s.cuda_stream))
        return out

    def witness_batch_position_major(self, chars, lens, out=None, stream=None, chars_pm_stride=None):
        """Like witness_batch, outputs in HRX_LAYOUT_POSITION_MAJOR (use position_major_to_string_major to view them per
        string).  chars: (B, stride) string-major, or — with chars_pm_stride=stride — the flat position-major buffer made by
        chars_to_position_major."""
        assert chars.is_cuda and lens.is_cuda and chars.dtype == torch.uint8 and lens.dtype == torch.int32
        layout = LAYOUT_POSITION_MAJOR
        if chars_pm_stride is None:
            assert chars.stride(1) == 1 and lens.is_contiguous()
            B, stride = chars.shape[0], chars.stride(0)
        else:
            assert chars.is_contiguous() and chars.numel() == lens.numel() * chars_pm_stride
            B, stride = lens.numel(), int(chars_pm_stride)
            layout |= LAYOUT_INPUT_POSITION_MAJOR
        if out is None:
            out = self.alloc_outputs_position_major(B, chars.device)
        rec, msk, st = out
        s = torch.cuda.current_stream(chars.device) if stream is None else stream
        _check(lib.hrx_witness_batch_device_layout(self._need_device(chars, lens, rec, msk, st), layout, chars.data_ptr(), stride,
                                                   lens.data_ptr(), B, self.max_chars_size, rec.data_ptr(), msk.data_ptr(),
                                                   st.data_ptr(), s.cuda_stream))
        return rec, msk, st

    def fr_columns(self, chars, lens, out, b_begin=0, b_count=None, position_major=False, chars_pm_stride=None, canonical=False,
                   stream=None, cells=None):
        """expand the compact rows `out` = (records, masked, status) of a finished witness_batch* call into
        bn256::Fr cells for strings [b_begin, b_begin + b_count): int64 CUDA tensor [4 + 4 D][b_count][M][4] (limbs).
        cells: the caller's contiguous int64 tensor of exactly that many elements, written in place and returned.  Type, contiguity and size are checked
        here; that it lies on this config's device is _need_device's check, and that it is 16-byte aligned the library's own (HrxError from either)."""
        rec, msk, _ = out
        B = lens.numel()
        b_count = B - b_begin if b_count is None else b_count
        M, D = self.max_chars_size, self.num_defs
        ncols = lib.hrx_fr_num_columns(D)
        if cells is None:
            cells = torch.empty((ncols, b_count, M, 4), dtype=torch.int64, device=lens.device)
        elif cells.dtype != torch.int64 or not cells.is_contiguous() or cells.numel() != ncols * b_count * M * 4:
            raise HrxError(HRX_ERR_ARG, "cells: a contiguous int64 tensor of [%d][%d][%d][4] elements" % (ncols, b_count, M))
        layout, rp, mp = LAYOUT_STRING_MAJOR, 0, 0
        if position_major:
            layout = LAYOUT_POSITION_MAJOR
            if chars_pm_stride is not None:
                layout |= LAYOUT_INPUT_POSITION_MAJOR
                stride = int(chars_pm_stride)
            else:
                stride = chars.stride(0)
        elif isinstance(rec, (list, tuple)):      # (record planes are a position-major layout: the library refuses)
            stride = chars.stride(0)
        else:
            stride, rp, mp = chars.stride(0), rec.stride(0) // D, msk.stride(0)
        s = torch.cuda.current_stream(lens.device) if stream is None else stream
        if isinstance(rec, (list, tuple)):      # record planes (or the two row stripes of one def)
            arr = (C.c_void_p * len(rec))(*[p.data_ptr() for p in rec])
            _check(lib.hrx_fr_columns_device_planes(self._need_device(chars, lens, msk, cells, *rec), layout, chars.data_ptr(), stride, lens.data_ptr(), arr, len(rec), msk.data_ptr(),
                                                    B, M, b_begin, b_count, cells.data_ptr(), FR_CANONICAL if canonical else 0, s.cuda_stream))
            return cells
        _check(lib.hrx_fr_columns_device(self._need_device(chars, lens, rec, msk, cells), layout, chars.data_ptr(), stride, lens.data_ptr(), rec.data_ptr(), rp,
                                         msk.data_ptr(), mp, B, M, b_begin, b_count, cells.data_ptr(),
                                         FR_CANONICAL if canonical else 0, s.cuda_stream))
        return cells

    def verify_chunk_rows(self, B, M=None):
        """hrx_ctx_verify_chunk_rows: the chunk the context picks for B strings of M rows (default: max_chars_size); >= M: one chunk, the plain launch is the better call"""
        return int(lib.hrx_ctx_verify_chunk_rows(self._need_ctx(), int(B), int(self.max_chars_size if M is None else M)))

    def verify_rows(self, chars, lens, records, masked, layout=LAYOUT_STRING_MAJOR, planes=None, rec_pitch=0, msk_pitch=0, out=None, chars_pm_stride=None,
                    stream=None, chunk_rows=None, workspace=None):
        """hrx_verify_rows_device / _planes: do the witness rows of a finished batch satisfy the circuit?  (B,) int64 CUDA tensor of verdict words (include/hrx.h VERIFY:
        0 = every gate, lookup and assignment rule holds; bits 0..8 VERIFY_*, bits 32..56 the lowest failing row — verdict_row / explain_verdict; -1: lens[b] > M).
        chars, lens and `layout` are those of the witness_batch* call that wrote the rows (chars_pm_stride: the flat position-major input and its per-string capacity);
        records / masked its outputs — string-major views, pitched or not (rec_pitch / msk_pitch in rows, 0: taken from a (B, M, D) / (B, M) view's strides), or the
        flat position-major buffers; planes: the list of record planes (or the two row stripes of one def) instead of records.  One launch, asynchronous on `stream`
        (default: torch's current stream); the context's first call also builds and uploads the check tables (not inside a graph capture).
        chunk_rows: None — that one launch; 0 or a multiple of 32 — hrx_verify_rows_chunked_device / _planes: the same words from chunks of that many rows (0: the
        context's pick, verify_chunk_rows), so that few long strings fill the device; two launches and a workspace of verify_chunked_workspace_bytes(B, M, chunk_rows)
        bytes — `workspace`, any contiguous CUDA tensor of at least that size, or one allocated here."""
        assert lens.is_cuda and lens.dtype == torch.int32 and lens.is_contiguous() and chars.dtype == torch.uint8
        B, M, D = lens.numel(), self.max_chars_size, self.num_defs
        stride, rec_pitch, msk_pitch = _torch_row_pitches(chars, None if planes is not None else records, masked, layout, D, rec_pitch, msk_pitch, chars_pm_stride)
        out = _out_buffer(out, "out", (B,), torch.int64, lens.device)
        s = torch.cuda.current_stream(lens.device) if stream is None else stream
        if chunk_rows is not None:
            chunk_rows = int(chunk_rows)
            need = verify_chunked_workspace_bytes(B, M, chunk_rows if chunk_rows else self.verify_chunk_rows(B))
            if workspace is None:
                workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=lens.device)
            ws_bytes = workspace.numel() * workspace.element_size()
            if planes is not None:
                arr = _planes_array(planes)
                _check(lib.hrx_verify_rows_chunked_device_planes(self._need_device(chars, lens, masked, out, workspace, *planes), int(layout), chars.data_ptr(), stride,
                                                                 lens.data_ptr(), arr, len(planes), masked.data_ptr(), B, M, chunk_rows, workspace.data_ptr(), ws_bytes,
                                                                 out.data_ptr(), s.cuda_stream))
                return out
            _check(lib.hrx_verify_rows_chunked_device(self._need_device(chars, lens, records, masked, out, workspace), int(layout), chars.data_ptr(), stride, lens.data_ptr(),
                                                      records.data_ptr(), int(rec_pitch), masked.data_ptr(), int(msk_pitch), B, M, chunk_rows, workspace.data_ptr(), ws_bytes,
                                                      out.data_ptr(), s.cuda_stream))
            return out
        if planes is not None:
            arr = _planes_array(planes)
            _check(lib.hrx_verify_rows_device_planes(self._need_device(chars, lens, masked, out, *planes), int(layout), chars.data_ptr(), stride, lens.data_ptr(), arr, len(planes),
                                                     masked.data_ptr(), B, M, out.data_ptr(), s.cuda_stream))
            return out
        _check(lib.hrx_verify_rows_device(self._need_device(chars, lens, records, masked, out), int(layout), chars.data_ptr(), stride, lens.data_ptr(), records.data_ptr(),
                                          int(rec_pitch), masked.data_ptr(), int(msk_pitch), B, M, out.data_ptr(), s.cuda_stream))
        return out

    def verify_rows_host(self, chars, lens, records, masked, layout=LAYOUT_STRING_MAJOR, rec_pitch=0, msk_pitch=0, out=None, chars_pm_stride=None, chunk_rows=None):
        """hrx_verify_rows_host: verify_rows over numpy arrays in host memory, on a host-only or a device context — the same rules (csrc/hrx_verify.hpp) over host
        threads; (B,) uint64.  String-major records (B, M, D) / masked (B, M) / chars (B, stride), pitched views included, or the flat position-major buffers.
        chunk_rows: None — that call; 0 or a multiple of 32 — hrx_verify_rows_chunked_host, the same words from the chunk walk and fold over (string, chunk) pairs."""
        lens = np.ascontiguousarray(lens, np.uint32)
        B, M, D = len(lens), self.max_chars_size, self.num_defs
        ch, rec, msk, stride, rec_pitch, msk_pitch = _numpy_rows(chars, records, masked, layout, D, rec_pitch, msk_pitch, chars_pm_stride)
        out = _out_buffer(out, "out", (B,), np.uint64)
        if chunk_rows is not None:
            _check(lib.hrx_verify_rows_chunked_host(self._need_ctx(), int(layout), ch.ctypes.data, stride, lens.ctypes.data, rec.ctypes.data, int(rec_pitch),
                                                    msk.ctypes.data, int(msk_pitch), B, M, int(chunk_rows), out.ctypes.data))
            return out
        _check(lib.hrx_verify_rows_host(self._need_ctx(), int(layout), ch.ctypes.data, stride, lens.ctypes.data, rec.ctypes.data, int(rec_pitch), msk.ctypes.data,
                                        int(msk_pitch), B, M, out.ctypes.data))
        return out

    def lookup_words(self):
        """hrx_lookup_words_per_string: the u32 words of one string's run of lookup counts (a multiple of 4)"""
        return int(lib.hrx_lookup_words_per_string(self._defs.h))

    def lookup_layout(self):
        """hrx_lookup_layout: per def a dict of slices into a string's run of lookup_words() counts — "trans" (one bin per row of load()[d][0]), "start" and
        "end" (one bin per row of load()[d][1] each)"""
        out = []
        for d in range(self.num_defs):
            v = [C.c_size_t() for _ in range(5)]
            _check(lib.hrx_lookup_layout(self._defs.h, d, *[C.byref(x) for x in v]))
            t_off, t_rows, s_off, e_off, e_rows = (int(x.value) for x in v)
            out.append({"trans": slice(t_off, t_off + t_rows), "start": slice(s_off, s_off + e_rows), "end": slice(e_off, e_off + e_rows)})
        return out

    def lookup_group(self, b_count):
        """hrx_ctx_lookup_group: (strings per workgroup, passes over the rows) of a lookup_counts call of b_count strings"""
        g, p = C.c_size_t(), C.c_size_t()
        _check(lib.hrx_ctx_lookup_group(self._need_ctx(), int(b_count), C.byref(g), C.byref(p)))
        return int(g.value), int(p.value)

    def lookup_counts(self, chars, lens, rec, layout=LAYOUT_STRING_MAJOR, planes=None, b_begin=0, b_count=None, out=None, misses=None, chars_pm_stride=None,
                      rec_pitch=0, stream=None):
        """hrx_lookup_counts_device / _planes: how often the witness rows of strings [b_begin, b_begin + b_count) of a finished batch hit each row of the three
        fixed lookup tables per def (include/hrx.h LOOKUP COUNTS).  Returns (counts, misses): (b_count, lookup_words()) and (b_count,) int32 CUDA tensors holding
        u32 bit patterns; lookup_layout() slices a counts row.  chars, lens, `layout`, rec / planes, rec_pitch and chars_pm_stride are verify_rows'.  out / misses: the
        caller's contiguous int32 tensors of exactly those sizes, written in place.  One launch, asynchronous on `stream` (default: torch's current stream); the
        context's first call also builds and uploads the image of the tables (not inside a graph capture)."""
        assert lens.is_cuda and lens.dtype == torch.int32 and lens.is_contiguous() and chars.dtype == torch.uint8
        B, M, D, W = lens.numel(), self.max_chars_size, self.num_defs, self.lookup_words()
        b_count = B - b_begin if b_count is None else int(b_count)
        stride, rec_pitch, _ = _torch_row_pitches(chars, None if planes is not None else rec, None, layout, D, rec_pitch, 0, chars_pm_stride)
        out = _out_buffer(out, "out", (b_count, W), torch.int32, lens.device)
        misses = _out_buffer(misses, "misses", (b_count,), torch.int32, lens.device)
        s = torch.cuda.current_stream(lens.device) if stream is None else stream
        if planes is not None:
            arr = _planes_array(planes)
            _check(lib.hrx_lookup_counts_device_planes(self._need_device(chars, lens, out, misses, *planes), int(layout), chars.data_ptr(), stride, lens.data_ptr(), arr,
                                                       len(planes), B, M, int(b_begin), b_count, out.data_ptr(), misses.data_ptr(), s.cuda_stream))
            return out, misses
        _check(lib.hrx_lookup_counts_device(self._need_device(chars, lens, rec, out, misses), int(layout), chars.data_ptr(), stride, lens.data_ptr(), rec.data_ptr(),
                                            int(rec_pitch), B, M, int(b_begin), b_count, out.data_ptr(), misses.data_ptr(), s.cuda_stream))
        return out, misses

    def lookup_counts_host(self, chars, lens, rec, layout=LAYOUT_STRING_MAJOR, b_begin=0, b_count=None, out=None, misses=None, chars_pm_stride=None, rec_pitch=0):
        """hrx_lookup_counts_host: lookup_counts over numpy arrays in host memory, on a host-only or a device context — the definition of the counts
        (csrc/hrx_lookup.hpp) over host threads.  Returns (counts (b_count, lookup_words()) uint32, misses (b_count,) uint32).  String-major records (B, M, D) /
        chars (B, stride), pitched views included, or the flat position-major buffers."""
        lens = np.ascontiguousarray(lens, np.uint32)
        B, M, D, W = len(lens), self.max_chars_size, self.num_defs, self.lookup_words()
        b_count = B - b_begin if b_count is None else int(b_count)
        ch, rec, _, stride, rec_pitch, _ = _numpy_rows(chars, rec, None, layout, D, rec_pitch, 0, chars_pm_stride)
        out = _out_buffer(out, "out", (b_count, W), np.uint32)
        misses = _out_buffer(misses, "misses", (b_count,), np.uint32)
        _check(lib.hrx_lookup_counts_host(self._need_ctx(), int(layout), ch.ctypes.data, stride, lens.ctypes.data, rec.ctypes.data, int(rec_pitch), B, M, int(b_begin),
                                          b_count, out.ctypes.data, misses.ctypes.data))
        return out, misses

    def lookup_compress_inputs(self, chars, lens, rec, theta, layout=LAYOUT_STRING_MAJOR, planes=None, b_begin=0, b_count=None, out=None, canonical=False,
                               chars_pm_stride=None, rec_pitch=0, stream=None):
        """hrx_lookup_compress_inputs_device / _planes: the three lookup tuples of every witness row of strings [b_begin, b_begin + b_count), folded with the
        challenge into bn256::Fr cells (include/hrx.h LOOKUP COMPRESS): int64 CUDA tensor [3 D][b_count][M][4] of limbs, column 3 d + k = the transition / start
        / end lookup of def d (FR_LOOKUP_COLUMN_NAMES).  theta: an int64 CUDA tensor of limbs, (b_count, 4) — one challenge per string — or (4,) — one for the
        call; Montgomery limbs in and out unless canonical.  chars, lens, `layout`, rec / planes, rec_pitch and chars_pm_stride are lookup_counts'.  out: the
        caller's contiguous int64 tensor of exactly that size, written in place.  One launch, asynchronous on `stream` (default: torch's current stream),
        capturable from the first call."""
        assert lens.is_cuda and lens.dtype == torch.int32 and lens.is_contiguous() and chars.dtype == torch.uint8
        B, M, D = lens.numel(), self.max_chars_size, self.num_defs
        b_count = B - b_begin if b_count is None else int(b_count)
        stride, rec_pitch, _ = _torch_row_pitches(chars, None if planes is not None else rec, None, layout, D, rec_pitch, 0, chars_pm_stride)
        theta_stride = _theta_stride(theta, b_count, torch.int64)
        out = _out_buffer(out, "out", (3 * D, b_count, M, 4), torch.int64, lens.device)
        s = torch.cuda.current_stream(lens.device) if stream is None else stream
        flags = FR_CANONICAL if canonical else 0
        if planes is not None:
            arr = _planes_array(planes)
            _check(lib.hrx_lookup_compress_inputs_device_planes(self._need_device(chars, lens, theta, out, *planes), int(layout), chars.data_ptr(), stride, lens.data_ptr(),
                                                                arr, len(planes), B, M, int(b_begin), b_count, theta.data_ptr(), theta_stride, out.data_ptr(), flags,
                                                                s.cuda_stream))
            return out
        _check(lib.hrx_lookup_compress_inputs_device(self._need_device(chars, lens, rec, theta, out), int(layout), chars.data_ptr(), stride, lens.data_ptr(), rec.data_ptr(),
                                                     int(rec_pitch), B, M, int(b_begin), b_count, theta.data_ptr(), theta_stride, out.data_ptr(), flags, s.cuda_stream))
        return out

    def lookup_compress_inputs_host(self, chars, lens, rec, theta, layout=LAYOUT_STRING_MAJOR, b_begin=0, b_count=None, out=None, canonical=False,
                                    chars_pm_stride=None, rec_pitch=0):
        """hrx_lookup_compress_inputs_host: lookup_compress_inputs over numpy arrays in host memory, on a host-only or a device context — the definition of the
        cells (csrc/hrx_compress.hpp) over host threads.  theta: uint64 limbs (b_count, 4) or (4,); returns uint64 [3 D][b_count][M][4]."""
        lens = np.ascontiguousarray(lens, np.uint32)
        B, M, D = len(lens), self.max_chars_size, self.num_defs
        b_count = B - b_begin if b_count is None else int(b_count)
        ch, rec, _, stride, rec_pitch, _ = _numpy_rows(chars, rec, None, layout, D, rec_pitch, 0, chars_pm_stride)
        theta = np.ascontiguousarray(theta, np.uint64)
        theta_stride = _theta_stride(theta, b_count, np.uint64)
        out = _out_buffer(out, "out", (3 * D, b_count, M, 4), np.uint64)
        _check(lib.hrx_lookup_compress_inputs_host(self._need_ctx(), int(layout), ch.ctypes.data, stride, lens.ctypes.data, rec.ctypes.data, int(rec_pitch), B, M,
                                                   int(b_begin), b_count, theta.ctypes.data, theta_stride, out.ctypes.data, FR_CANONICAL if canonical else 0))
        return out

    def lookup_compress_table(self, theta, out=None, canonical=False, stream=None):
        """hrx_lookup_compress_table_device: the rows of the fixed lookup tables folded with each challenge, in the index space of the counts: int64 CUDA tensor
        [n_theta][lookup_words()][4] — cell w of a run is the compressed table row lookup_counts' word w counts (lookup_layout() slices a run; the start and end
        runs hold equal cells; pad words are zero cells).  theta: int64 CUDA limbs (n_theta, 4) or (4,) (one run).  The context's first call also builds and
        uploads the tables' tuples (not inside a graph capture)."""
        W = self.lookup_words()
        n_theta = 1 if theta.dim() == 1 else theta.shape[0]
        _theta_stride(theta, n_theta, torch.int64)
        out = _out_buffer(out, "out", (n_theta, W, 4), torch.int64, theta.device)
        s = torch.cuda.current_stream(theta.device) if stream is None else stream
        _check(lib.hrx_lookup_compress_table_device(self._need_device(theta, out), theta.data_ptr(), 4, n_theta, out.data_ptr(), FR_CANONICAL if canonical else 0,
                                                    s.cuda_stream))
        return out

    def lookup_compress_table_host(self, theta, out=None, canonical=False):
        """hrx_lookup_compress_table_host: lookup_compress_table over numpy arrays — theta uint64 limbs (n_theta, 4) or (4,); uint64 [n_theta][lookup_words()][4]"""
        W = self.lookup_words()
        theta = np.ascontiguousarray(theta, np.uint64)
        n_theta = 1 if theta.ndim == 1 else theta.shape[0]
        _theta_stride(theta, n_theta, np.uint64)
        out = _out_buffer(out, "out", (n_theta, W, 4), np.uint64)
        _check(lib.hrx_lookup_compress_table_host(self._need_ctx(), theta.ctypes.data, 4, n_theta, out.ctypes.data, FR_CANONICAL if canonical else 0))
        return out

    def lookup_permute_workspace_bytes(self, b_count, n_rows):
        """hrx_lookup_permute_workspace_bytes: the device workspace of a lookup_permute call (0 unless a table has more rows than the kernel keeps in LDS)"""
        return int(lib.hrx_lookup_permute_workspace_bytes(self._defs.h, int(b_count), int(n_rows)))

    def lookup_permute_plan(self, b_count, n_rows):
        """hrx_ctx_lookup_permute_plan: how a lookup_permute call cuts its work — a dict of tile_rows (positions of one expansion step), chunk_rows (table rows
        held in LDS at once), group_rows (positions per workgroup) and groups (workgroups per (string, lookup))"""
        v = [C.c_size_t() for _ in range(4)]
        _check(lib.hrx_ctx_lookup_permute_plan(self._need_ctx(), int(b_count), int(n_rows), *[C.byref(x) for x in v]))
        return dict(zip(("tile_rows", "chunk_rows", "group_rows", "groups"), (int(x.value) for x in v)))

    def lookup_permute(self, counts, n_rows, table=None, pitch=0, out=("idx", "cells"), overflow=True, workspace=None, stream=None):
        """hrx_lookup_permute_device: the permuted columns A', S' of halo2's lookup argument out of lookup_counts' counts, no sort (include/hrx.h LOOKUP
        PERMUTE).  counts: (b_count, lookup_words()) int32 CUDA tensor.  Returns a dict: "a_idx", "s_idx" — int32 [3 D][b_count][pitch] word indices into a
        string's run (the index space of the counts and of lookup_compress_table) — where "idx" is in `out`; "a_cells", "s_cells" — int64
        [3 D][b_count][pitch][4], the table cells at those indices — where `table` is given and "cells" is in `out`; "overflow" — int32 (b_count,), bit
        3 d + k where that lookup's counts exceed n_rows (its indices are 0xffffffff, its cells 0) — unless overflow is False.  table: lookup_compress_table's
        int64 tensor, (W, 4) — one run for the call — or (b_count, W, 4).  pitch: a multiple of 4, at least n_rows (0: n_rows rounded up); entries
        [n_rows, pitch) are never written.  `out` may also be a dict of the caller's contiguous tensors under those names (and "overflow"), written in place.
        workspace: an int8 CUDA tensor of lookup_permute_workspace_bytes() bytes (allocated where needed and not given).  One launch (two with overflow),
        asynchronous on `stream` (default: torch's current stream), capturable from the first call."""
        assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous()
        s = torch.cuda.current_stream(counts.device) if stream is None else stream

        def call(b_count, pitch, a_idx, s_idx, table, table_stride, a_cells, s_cells, ov):
            ws = workspace
            need = self.lookup_permute_workspace_bytes(b_count, n_rows)
            if ws is None and need:
                ws = torch.empty(need, dtype=torch.int8, device=counts.device)
            ptr = lambda t: t.data_ptr() if t is not None else None
            return lib.hrx_lookup_permute_device(self._need_device(counts, a_idx, s_idx, table, a_cells, s_cells, ov, ws), counts.data_ptr(), b_count, int(n_rows),
                                                 pitch, ptr(a_idx), ptr(s_idx), ptr(table), table_stride, ptr(a_cells), ptr(s_cells), ptr(ov), ptr(ws),
                                                 ws.numel() if ws is not None else 0, s.cuda_stream)

        return self._lookup_permute(counts, n_rows, table, pitch, out, overflow, torch.int32, torch.int64, counts.device, call)

    def lookup_permute_host(self, counts, n_rows, table=None, pitch=0, out=("idx", "cells"), overflow=True):
        """hrx_lookup_permute_host: lookup_permute over numpy arrays in host memory, on a host-only or a device context — the definition of the columns
        (csrc/hrx_permute.hpp) over host threads.  counts uint32 (b_count, lookup_words()); table uint64 (W, 4) or (b_count, W, 4); the dict's arrays are
        uint32 / uint64.  Entries [n_rows, pitch) are never written (arrays allocated here hold zeros there)."""
        counts = np.ascontiguousarray(counts, np.uint32)
        table = None if table is None else np.ascontiguousarray(table, np.uint64)

        def call(b_count, pitch, a_idx, s_idx, table, table_stride, a_cells, s_cells, ov):
            ptr = lambda t: t.ctypes.data if t is not None else None
            return lib.hrx_lookup_permute_host(self._need_ctx(), counts.ctypes.data, b_count, int(n_rows), pitch, ptr(a_idx), ptr(s_idx), ptr(table), table_stride,
                                               ptr(a_cells), ptr(s_cells), ptr(ov))

        return self._lookup_permute(counts, n_rows, table, pitch, out, overflow, np.uint32, np.uint64, None, call)

    def _lookup_permute(self, counts, n_rows, table, pitch, out, overflow, u32, u64, device, call):
        """what lookup_permute (torch: u32 / u64 are torch.int32 / torch.int64, buffers on `device`) and lookup_permute_host (numpy, device None) share: which
        outputs the caller wants, their buffers — the caller's or fresh ones; numpy's zeroed — and the call: call(b_count, pitch, a_idx, s_idx, table,
        table_stride, a_cells, s_cells, overflow) with None for what is not wanted"""
        W, ncols = self.lookup_words(), 3 * self.num_defs
        size = counts.numel() if device is not None else counts.size
        b_count = size // W if W else 0
        if size != b_count * W:
            raise HrxError(HRX_ERR_ARG, "counts: a contiguous 32-bit array or tensor of [b_count][%d] elements" % W)
        n_rows, pitch = int(n_rows), int(pitch)
        p = pitch if pitch else (n_rows + 3) & ~3
        given = out if isinstance(out, dict) else {}
        want_idx = "a_idx" in given if given else "idx" in out
        want_cells = "a_cells" in given if given else (table is not None and "cells" in out)
        res = {}

        def buf(name, shape, dtype):
            res[name] = _out_buffer(given.get(name), name, shape, dtype, device, zeros=True)
            return res[name]

        a_idx = s_idx = a_cells = s_cells = ov = None
        if want_idx:
            a_idx, s_idx = buf("a_idx", (ncols, b_count, p), u32), buf("s_idx", (ncols, b_count, p), u32)
        if want_cells:
            contiguous = table is not None and (table.is_contiguous() if device is not None else table.flags.c_contiguous)
            if not contiguous or table.dtype != u64 or tuple(table.shape) not in ((W, 4), (b_count, W, 4)):
                raise HrxError(HRX_ERR_ARG, "table: contiguous 64-bit limbs of shape [%d][4] or [%d][%d][4]" % (W, b_count, W))
            a_cells, s_cells = buf("a_cells", (ncols, b_count, p, 4), u64), buf("s_cells", (ncols, b_count, p, 4), u64)
        else:
            table = None
        if overflow or "overflow" in given:
            ov = buf("overflow", (b_count,), u32)
        _check(call(b_count, pitch, a_idx, s_idx, table, 4 * W if table is not None and len(table.shape) == 3 else 0, a_cells, s_cells, ov))
        return res

    def lookup_invert_workspace_bytes(self, n_runs):
        """hrx_lookup_invert_workspace_bytes: the device workspace of a lookup_invert_table call (0 in this build: a run is inverted inside one workgroup)"""
        return int(lib.hrx_lookup_invert_workspace_bytes(self._defs.h, int(n_runs)))

    def lookup_invert_table(self, table, shift, out=None, canonical=False, workspace=None, stream=None):
        """hrx_lookup_invert_table_device: 1 / (S + shift) for every cell of lookup_compress_table's runs (include/hrx.h LOOKUP PRODUCT): table int64 CUDA limbs
        (n_runs, W, 4) or (W, 4); shift int64 CUDA limbs (n_runs, 4) — one per run — or (4,) — one for the call.  Returns int64 limbs of table's shape: the zero
        cell where S + shift is zero and in the pad words.  Montgomery limbs in and out unless canonical.  workspace: an int8 CUDA tensor of
        lookup_invert_workspace_bytes() bytes (allocated where needed and not given).  One launch, asynchronous on `stream` (default: torch's current stream),
        capturable from the first call."""
        W = self.lookup_words()
        assert table.is_cuda and table.dtype == torch.int64 and table.is_contiguous()
        if tuple(table.shape[-2:]) != (W, 4) or table.dim() not in (2, 3):
            raise HrxError(HRX_ERR_ARG, "table: contiguous 64-bit limbs of shape [%d][4] or [n_runs][%d][4]" % (W, W))
        n_runs = 1 if table.dim() == 2 else table.shape[0]
        stride = _theta_stride(shift, n_runs, torch.int64)
        out = _out_buffer(out, "out", tuple(table.shape), torch.int64, table.device)
        ws = workspace
        need = self.lookup_invert_workspace_bytes(n_runs)
        if ws is None and need:
            ws = torch.empty(need, dtype=torch.int8, device=table.device)
        s = torch.cuda.current_stream(table.device) if stream is None else stream
        _check(lib.hrx_lookup_invert_table_device(self._need_device(table, shift, out, ws), table.data_ptr(), n_runs, shift.data_ptr(), stride, out.data_ptr(),
                                                  FR_CANONICAL if canonical else 0, ws.data_ptr() if ws is not None else None,
                                                  ws.numel() if ws is not None else 0, s.cuda_stream))
        return out

    def lookup_invert_table_host(self, table, shift, out=None, canonical=False):
        """hrx_lookup_invert_table_host: lookup_invert_table over numpy arrays — table uint64 (n_runs, W, 4) or (W, 4), shift uint64 (n_runs, 4) or (4,); the
        definition of the inverse cells (csrc/hrx_product.hpp) over host threads"""
        W = self.lookup_words()
        table = np.ascontiguousarray(table, np.uint64)
        shift = np.ascontiguousarray(shift, np.uint64)
        if tuple(table.shape[-2:]) != (W, 4) or table.ndim not in (2, 3):
            raise HrxError(HRX_ERR_ARG, "table: 64-bit limbs of shape [%d][4] or [n_runs][%d][4]" % (W, W))
        n_runs = 1 if table.ndim == 2 else table.shape[0]
        stride = _theta_stride(shift, n_runs, np.uint64)
        out = _out_buffer(out, "out", tuple(table.shape), np.uint64)
        _check(lib.hrx_lookup_invert_table_host(self._need_ctx(), table.ctypes.data, n_runs, shift.ctypes.data, stride, out.ctypes.data,
                                                FR_CANONICAL if canonical else 0))
        return out

    def lookup_product_plan(self, b_count, n_rows):
        """hrx_ctx_lookup_product_plan: how a lookup_product call cuts its work — a dict of tile_rows (entries of a Z column a workgroup takes per step) and
        rows_per_lane (consecutive entries per lane)"""
        v = [C.c_size_t() for _ in range(2)]
        _check(lib.hrx_ctx_lookup_product_plan(self._need_ctx(), int(b_count), int(n_rows), *[C.byref(x) for x in v]))
        return dict(zip(("tile_rows", "rows_per_lane"), (int(x.value) for x in v)))

    def lookup_product(self, lens, in_cells, a_idx, s_idx, n_rows, table, inv_beta, inv_gamma, beta, gamma, b_begin=0, z_pitch=0, canonical=False, open=True,
                       out=None, stream=None):
        """hrx_lookup_product_device: the grand product Z of halo2's lookup argument for every lookup of the strings [b_begin, b_begin + b_count) (include/hrx.h
        LOOKUP PRODUCT).  lens: the batch's int32 CUDA tensor; in_cells: lookup_compress_inputs' int64 [3 D][b_count][M][4]; a_idx, s_idx: lookup_permute's int32
        [3 D][b_count][idx_pitch]; table, inv_beta, inv_gamma: int64 limbs, all three (W, 4) — one run for the call — or (b_count, W, 4); beta, gamma: int64
        limbs (4,) or (b_count, 4), alike.  Returns {"z": int64 [3 D][b_count][z_pitch][4] — entries [0, n_rows] written, the others never; "open": int32
        (b_count,), bit 3 d + k where Z[n_rows] != 1 (unless open is False)}.  z_pitch: a multiple of 4 above n_rows (0: n_rows + 1 rounded up).  `out`: a dict
        of the caller's contiguous tensors under those names, written in place.  One launch (two with open), asynchronous on `stream` (default: torch's current
        stream), capturable from the first call."""
        assert lens.is_cuda and lens.dtype == torch.int32 and lens.is_contiguous()
        s = torch.cuda.current_stream(lens.device) if stream is None else stream

        def call(b_count, idx_pitch, table_stride, challenge_stride, z, zp, op):
            ptr = lambda t: t.data_ptr() if t is not None else None
            return lib.hrx_lookup_product_device(self._need_device(lens, in_cells, a_idx, s_idx, table, inv_beta, inv_gamma, beta, gamma, z, op), lens.data_ptr(),
                                                 self.max_chars_size, int(b_begin), b_count, in_cells.data_ptr(), a_idx.data_ptr(), s_idx.data_ptr(), int(n_rows),
                                                 idx_pitch, table.data_ptr(), inv_beta.data_ptr(), inv_gamma.data_ptr(), table_stride, beta.data_ptr(),
                                                 gamma.data_ptr(), challenge_stride, z.data_ptr(), zp, ptr(op), FR_CANONICAL if canonical else 0, s.cuda_stream)

        return self._lookup_product(in_cells, a_idx, s_idx, n_rows, table, inv_beta, inv_gamma, beta, gamma, z_pitch, open, out, torch.int32, torch.int64,
                                    lens.device, call)

    def lookup_product_host(self, lens, in_cells, a_idx, s_idx, n_rows, table, inv_beta, inv_gamma, beta, gamma, b_begin=0, z_pitch=0, canonical=False, open=True,
                            out=None):
        """hrx_lookup_product_host: lookup_product over numpy arrays in host memory (uint32 / uint64), on a host-only or a device context — the definition of
        Z (csrc/hrx_product.hpp) over host threads.  Entries above n_rows are never written (arrays allocated here hold zeros there)."""
        lens = np.ascontiguousarray(lens, np.uint32)
        in_cells, table, inv_beta, inv_gamma, beta, gamma = (np.ascontiguousarray(x, np.uint64) for x in (in_cells, table, inv_beta, inv_gamma, beta, gamma))
        a_idx, s_idx = np.ascontiguousarray(a_idx, np.uint32), np.ascontiguousarray(s_idx, np.uint32)

        def call(b_count, idx_pitch, table_stride, challenge_stride, z, zp, op):
            return lib.hrx_lookup_product_host(self._need_ctx(), lens.ctypes.data, self.max_chars_size, int(b_begin), b_count, in_cells.ctypes.data, a_idx.ctypes.data,
                                               s_idx.ctypes.data, int(n_rows), idx_pitch, table.ctypes.data, inv_beta.ctypes.data, inv_gamma.ctypes.data, table_stride,
                                               beta.ctypes.data, gamma.ctypes.data, challenge_stride, z.ctypes.data, zp, op.ctypes.data if op is not None else None,
                                               FR_CANONICAL if canonical else 0)

        return self._lookup_product(in_cells, a_idx, s_idx, n_rows, table, inv_beta, inv_gamma, beta, gamma, z_pitch, open, out, np.uint32, np.uint64, None, call)

    def _lookup_product(self, in_cells, a_idx, s_idx, n_rows, table, inv_beta, inv_gamma, beta, gamma, z_pitch, open, out, u32, u64, device, call):
        """what lookup_product (torch) and lookup_product_host (numpy, device None) share: the shapes, the strides, the output buffers — the caller's or fresh
        ones; numpy's zeroed — and the call: call(b_count, idx_pitch, table_stride, challenge_stride, z, z_pitch, open)"""
        W, ncols, M = self.lookup_words(), 3 * self.num_defs, self.max_chars_size
        contiguous = lambda t: t.is_contiguous() if device is not None else t.flags.c_contiguous
        if in_cells.dtype != u64 or not contiguous(in_cells) or len(in_cells.shape) != 4 or tuple(in_cells.shape[0:1] + in_cells.shape[2:]) != (ncols, M, 4):
            raise HrxError(HRX_ERR_ARG, "in_cells: contiguous 64-bit limbs of shape [%d][b_count][%d][4]" % (ncols, M))
        b_count = in_cells.shape[1]
        for name, t in (("a_idx", a_idx), ("s_idx", s_idx)):
            if t.dtype != u32 or not contiguous(t) or len(t.shape) != 3 or tuple(t.shape[:2]) != (ncols, b_count) or tuple(t.shape) != tuple(a_idx.shape):
                raise HrxError(HRX_ERR_ARG, "%s: contiguous 32-bit words of shape [%d][%d][idx_pitch]" % (name, ncols, b_count))
        for name, t in (("table", table), ("inv_beta", inv_beta), ("inv_gamma", inv_gamma)):
            if t.dtype != u64 or not contiguous(t) or tuple(t.shape) not in ((W, 4), (b_count, W, 4)) or tuple(t.shape) != tuple(table.shape):
                raise HrxError(HRX_ERR_ARG, "%s: contiguous 64-bit limbs of shape [%d][4] or [%d][%d][4], the three alike" % (name, W, b_count, W))
        if _theta_stride(beta, b_count, u64) != _theta_stride(gamma, b_count, u64):
            raise HrxError(HRX_ERR_ARG, "beta and gamma: both (4,) or both (%d, 4)" % b_count)
        n_rows, z_pitch = int(n_rows), int(z_pitch)
        p = z_pitch if z_pitch else (n_rows + 4) & ~3
        given = out if isinstance(out, dict) else {}
        res = {"z": _out_buffer(given.get("z"), "z", (ncols, b_count, p, 4), u64, device, zeros=True)}
        if open or "open" in given:
            res["open"] = _out_buffer(given.get("open"), "open", (b_count,), u32, device, zeros=True)
        _check(call(b_count, a_idx.shape[2], 4 * W if len(table.shape) == 3 else 0, _theta_stride(beta, b_count, u64), res["z"], z_pitch, res.get("open")))
        return res

    def fr_ntt_workspace_bytes(self, k):
        """hrx_fr_ntt_workspace_bytes: the device workspace of the transforms of size 2^k (the twiddle table and 2^-k); 0 for a k out of range"""
        return int(lib.hrx_fr_ntt_workspace_bytes(int(k)))

    def fr_ntt_plan(self, n_cols, k):
        """hrx_ctx_fr_ntt_plan: how a device transform cuts its work — a dict of n_passes, pass_bits (a list of n_passes stage counts, their sum k) and
        cols_per_group (whole columns a workgroup takes where the call is one pass)"""
        n, cpg, bits = C.c_size_t(), C.c_size_t(), (C.c_size_t * 3)()
        _check(lib.hrx_ctx_fr_ntt_plan(self._need_ctx(), int(n_cols), int(k), C.byref(n), bits, C.byref(cpg)))
        return {"n_passes": int(n.value), "pass_bits": [int(b) for b in bits[:n.value]], "cols_per_group": int(cpg.value)}

    def fr_ntt_prepare(self, k, workspace=None, stream=None):
        """hrx_fr_ntt_prepare_device: write the tables of size 2^k into `workspace` — an int8 CUDA tensor of fr_ntt_workspace_bytes(k) bytes, allocated where
        not given — in one launch, asynchronous on `stream` (default: torch's current stream).  Returns the workspace: read-only from then on, for any
        number of fr_ntt calls of that k."""
        device = torch.device("cuda", self.device) if workspace is None else workspace.device
        ws = torch.empty(max(self.fr_ntt_workspace_bytes(k), 1), dtype=torch.int8, device=device) if workspace is None else workspace
        s = torch.cuda.current_stream(device) if stream is None else stream
        _check(lib.hrx_fr_ntt_prepare_device(self._need_device(ws), int(k), ws.data_ptr(), ws.numel() * ws.element_size(), s.cuda_stream))
        return ws

    def fr_ntt(self, cells, k, workspace=None, out=None, inverse=False, n_in=None, shift=None, canonical=False, stream=None):
        """hrx_fr_ntt_device: the transform of size 2^k of every column of `cells` (include/hrx.h FR NTT) — int64 CUDA limbs (n_cols, in_pitch, 4) or
        (in_pitch, 4), entries [0, n_in) of a column read (n_in: default min(in_pitch, 2^k)), the others zero and never read.  forward:
        y[j] = sum_i shift^i x[i] w^(i j); inverse=True: y[i] = shift^i 2^-k sum_j x[j] w^(-i j).  shift: int64 CUDA limbs (4,), or None (1).  Returns int64
        limbs (n_cols, out_pitch, 4) (or (out_pitch, 4)): `out` if given — the caller's contiguous tensor, out_pitch >= 2^k, entries above 2^k never
        written; `out is cells`: in place — else a fresh tensor of pitch 2^k (4 for k = 1).  Montgomery limbs unless canonical.  workspace: fr_ntt_prepare(k)'s (prepared
        here where not given: one more launch).  Asynchronous on `stream` (default: torch's current stream), capturable from the first call."""
        assert cells.is_cuda and cells.dtype == torch.int64 and cells.is_contiguous()
        s = torch.cuda.current_stream(cells.device) if stream is None else stream
        ws = self.fr_ntt_prepare(k, stream=s) if workspace is None else workspace

        def call(n_cols, in_pitch, out, out_pitch, n_in, flags):
            return lib.hrx_fr_ntt_device(self._need_device(cells, out, shift, ws), cells.data_ptr(), in_pitch, out.data_ptr(), out_pitch, n_cols, int(k), n_in,
                                         shift.data_ptr() if shift is not None else None, flags, ws.data_ptr(), ws.numel() * ws.element_size(), s.cuda_stream)

        return self._fr_ntt(cells, k, out, inverse, n_in, shift, canonical, torch.int64, cells.device, call)

    def fr_ntt_host(self, cells, k, out=None, inverse=False, n_in=None, shift=None, canonical=False):
        """hrx_fr_ntt_host: fr_ntt over numpy arrays in host memory (uint64), on a host-only or a device context — the definition of the cells
        (csrc/hrx_ntt.hpp), an iterative radix-2 transform per column over host threads; no workspace.  Entries above 2^k of a caller's `out` are never
        written."""
        if out is not None and out is cells:
            assert cells.dtype == np.uint64 and cells.flags.c_contiguous
        else:
            cells = np.ascontiguousarray(cells, np.uint64)
        shift = None if shift is None else np.ascontiguousarray(shift, np.uint64)

        def call(n_cols, in_pitch, out, out_pitch, n_in, flags):
            return lib.hrx_fr_ntt_host(self._need_ctx(), cells.ctypes.data, in_pitch, out.ctypes.data, out_pitch, n_cols, int(k), n_in,
                                       shift.ctypes.data if shift is not None else None, flags)

        return self._fr_ntt(cells, k, out, inverse, n_in, shift, canonical, np.uint64, None, call)

    def _fr_ntt(self, cells, k, out, inverse, n_in, shift, canonical, u64, device, call):
        """what fr_ntt (torch) and fr_ntt_host (numpy, device None) share: the shapes, the output buffer — the caller's or a fresh one of pitch 2^k — and the
        call: call(n_cols, in_pitch, out, out_pitch, n_in, flags)"""
        k = int(k)
        contiguous = lambda t: t.is_contiguous() if device is not None else t.flags.c_contiguous
        if cells.dtype != u64 or len(cells.shape) not in (2, 3) or cells.shape[-1] != 4:
            raise HrxError(HRX_ERR_ARG, "cells: contiguous 64-bit limbs of shape [n_cols][in_pitch][4] or [in_pitch][4]")
        if not 1 <= k <= 24:
            raise HrxError(HRX_ERR_ARG, "k: 1 .. 24")
        n_cols, in_pitch = (1, cells.shape[0]) if len(cells.shape) == 2 else (cells.shape[0], cells.shape[1])
        n_in = min(in_pitch, 1 << k) if n_in is None else int(n_in)
        if shift is not None and (shift.dtype != u64 or not contiguous(shift) or tuple(shift.shape) != (4,)):
            raise HrxError(HRX_ERR_ARG, "shift: contiguous 64-bit limbs of shape (4,)")
        if out is None:
            out = _out_buffer(None, "out", tuple(cells.shape[:-2]) + (max(1 << k, 4), 4), u64, device, zeros=True)
        elif out.dtype != u64 or not contiguous(out) or len(out.shape) != len(cells.shape) or out.shape[-1] != 4 or tuple(out.shape[:-2]) != tuple(cells.shape[:-2]):
            raise HrxError(HRX_ERR_ARG, "out: contiguous 64-bit limbs of shape [n_cols][out_pitch][4], as many columns as cells has")
        _check(call(n_cols, in_pitch, out, out.shape[-2], n_in, (FR_CANONICAL if canonical else 0) | (FR_NTT_INVERSE if inverse else 0)))
        return out

    def lookup_quotient_plan(self, b_count, ext_k):
        """hrx_ctx_lookup_quotient_plan: how a lookup_quotient call cuts its work — a dict of tile_cells (consecutive points of one string a workgroup takes)
        and cells_per_lane"""
        v = [C.c_size_t() for _ in range(2)]
        _check(lib.hrx_ctx_lookup_quotient_plan(self._need_ctx(), int(b_count), int(ext_k), *[C.byref(x) for x in v]))
        return dict(zip(("tile_cells", "cells_per_lane"), (int(x.value) for x in v)))

    def fr_vanishing_inverse(self, k, ext_k, shift=None, out=None, canonical=False, stream=None):
        """hrx_fr_vanishing_inverse_device: t_inv[c] = 1 / (g^(2^k) w_ext^(2^k c) - 1), c < 2^(ext_k - k) — what X^n - 1 takes on the extended coset of
        generator g, inverted; the zero cell where that is zero (include/hrx.h LOOKUP QUOTIENT).  shift: g as int64 CUDA limbs (4,), or None (1).  Returns int64
        limbs (2^(ext_k - k), 4) on the config's device (`out` if given).  Montgomery limbs unless canonical.  One launch of one workgroup, asynchronous on
        `stream` (default: torch's current stream), capturable from the first call."""
        device = torch.device("cuda", self.device) if shift is None else shift.device
        s = torch.cuda.current_stream(device) if stream is None else stream
        rot = 1 << max(int(ext_k) - int(k), 0)
        out = _out_buffer(out, "out", (rot, 4), torch.int64, device)
        _check(lib.hrx_fr_vanishing_inverse_device(self._need_device(shift, out), int(k), int(ext_k), shift.data_ptr() if shift is not None else None,
                                                   out.data_ptr(), FR_CANONICAL if canonical else 0, s.cuda_stream))
        return out

    def fr_vanishing_inverse_host(self, k, ext_k, shift=None, out=None, canonical=False):
        """hrx_fr_vanishing_inverse_host: fr_vanishing_inverse over numpy arrays (uint64), on a host-only or a device context — the definition of the table
        (csrc/hrx_quotient.hpp)"""
        shift = None if shift is None else np.ascontiguousarray(shift, np.uint64)
        out = _out_buffer(out, "out", (1 << max(int(ext_k) - int(k), 0), 4), np.uint64)
        _check(lib.hrx_fr_vanishing_inverse_host(self._need_ctx(), int(k), int(ext_k), shift.ctypes.data if shift is not None else None, out.ctypes.data,
                                                 FR_CANONICAL if canonical else 0))
        return out

    def lookup_quotient(self, k, ext_k, a_ext, ap_ext, sp_ext, z_ext, s_ext, selectors, beta, gamma, y, h_in=None, out=None, t_inv=None, divide=False,
                        canonical=False, stream=None):
        """hrx_lookup_quotient_device: the five constraints of every lookup at every point of the extended coset, folded into the quotient accumulator with y
        (include/hrx.h LOOKUP QUOTIENT).  a_ext, ap_ext, sp_ext, z_ext: int64 CUDA limbs [3 D][b_count][pitch][4] — A, A', S', Z on the coset (fr_ntt at ext_k
        with the coset's generator); s_ext: [3 D][s_pitch][4] — one table run for the call — or [3 D][b_count][s_pitch][4]; selectors: [3][sel_pitch][4]
        (lookup_quotient_selectors); beta, gamma, y: int64 limbs (4,) or (b_count, 4), the three alike; h_in: [b_count][h_pitch][4] or None (zero).  Returns
        h_out, int64 [b_count][h_pitch][4]: `out` if given (`out is h_in`: in place), else a fresh tensor of pitch 2^ext_k; entries [0, 2^ext_k) of a column
        written, the others never.  divide=True: times t_inv (fr_vanishing_inverse), the division by X^n - 1.  Montgomery limbs unless canonical.  One
        launch, asynchronous on `stream` (default: torch's current stream), capturable from the first call."""
        assert z_ext.is_cuda and z_ext.dtype == torch.int64
        s = torch.cuda.current_stream(z_ext.device) if stream is None else stream

        def call(b_count, pitch, s_pitch, s_stride, sel_pitch, challenge_stride, h_out, h_pitch, flags):
            ptr = lambda t: t.data_ptr() if t is not None else None
            return lib.hrx_lookup_quotient_device(self._need_device(a_ext, ap_ext, sp_ext, z_ext, s_ext, selectors, beta, gamma, y, h_in, h_out, t_inv), b_count, int(k),
                                                  int(ext_k), a_ext.data_ptr(), ap_ext.data_ptr(), sp_ext.data_ptr(), z_ext.data_ptr(), pitch, s_ext.data_ptr(), s_pitch,
                                                  s_stride, selectors.data_ptr(), sel_pitch, beta.data_ptr(), gamma.data_ptr(), y.data_ptr(), challenge_stride,
                                                  ptr(h_in), h_out.data_ptr(), h_pitch, ptr(t_inv), flags, s.cuda_stream)

        return self._lookup_quotient(ext_k, a_ext, ap_ext, sp_ext, z_ext, s_ext, selectors, beta, gamma, y, h_in, out, t_inv, divide, canonical, torch.int64,
                                     z_ext.device, call)

    def lookup_quotient_host(self, k, ext_k, a_ext, ap_ext, sp_ext, z_ext, s_ext, selectors, beta, gamma, y, h_in=None, out=None, t_inv=None, divide=False,
                             canonical=False):
        """hrx_lookup_quotient_host: lookup_quotient over numpy arrays in host memory (uint64), on a host-only or a device context — the definition of the
        cells (csrc/hrx_quotient.hpp) over host threads by ranges of strings.  Entries above 2^ext_k of a caller's `out` are never written."""
        a_ext, ap_ext, sp_ext, z_ext, s_ext, selectors, beta, gamma, y = (np.ascontiguousarray(x, np.uint64)
                                                                          for x in (a_ext, ap_ext, sp_ext, z_ext, s_ext, selectors, beta, gamma, y))
        t_inv = None if t_inv is None else np.ascontiguousarray(t_inv, np.uint64)
        if h_in is not None and h_in is not out:
            h_in = np.ascontiguousarray(h_in, np.uint64)

        def call(b_count, pitch, s_pitch, s_stride, sel_pitch, challenge_stride, h_out, h_pitch, flags):
            ptr = lambda t: t.ctypes.data if t is not None else None
            return lib.hrx_lookup_quotient_host(self._need_ctx(), b_count, int(k), int(ext_k), a_ext.ctypes.data, ap_ext.ctypes.data, sp_ext.ctypes.data,
                                                z_ext.ctypes.data, pitch, s_ext.ctypes.data, s_pitch, s_stride, selectors.ctypes.data, sel_pitch, beta.ctypes.data,
                                                gamma.ctypes.data, y.ctypes.data, challenge_stride, ptr(h_in), h_out.ctypes.data, h_pitch, ptr(t_inv), flags)

        return self._lookup_quotient(ext_k, a_ext, ap_ext, sp_ext, z_ext, s_ext, selectors, beta, gamma, y, h_in, out, t_inv, divide, canonical, np.uint64, None, call)

    def _lookup_quotient(self, ext_k, a_ext, ap_ext, sp_ext, z_ext, s_ext, selectors, beta, gamma, y, h_in, out, t_inv, divide, canonical, u64, device, call):
        """what lookup_quotient (torch) and lookup_quotient_host (numpy, device None) share: the shapes, the strides, the output buffer — the caller's or a fresh
        one of pitch 2^ext_k — and the call: call(b_count, pitch, s_pitch, s_stride, sel_pitch, challenge_stride, h_out, h_pitch, flags)"""
        ncols = 3 * self.num_defs
        contiguous = lambda t: t.is_contiguous() if device is not None else t.flags.c_contiguous
        for name, t in (("a_ext", a_ext), ("ap_ext", ap_ext), ("sp_ext", sp_ext), ("z_ext", z_ext)):
            if t.dtype != u64 or not contiguous(t) or len(t.shape) != 4 or t.shape[0] != ncols or t.shape[3] != 4 or tuple(t.shape) != tuple(z_ext.shape):
                raise HrxError(HRX_ERR_ARG, "%s: contiguous 64-bit limbs of shape [%d][b_count][pitch][4], the four alike" % (name, ncols))
        b_count, pitch = z_ext.shape[1], z_ext.shape[2]
        if s_ext.dtype != u64 or not contiguous(s_ext) or s_ext.shape[0] != ncols or s_ext.shape[-1] != 4 or \
                not (len(s_ext.shape) == 3 or (len(s_ext.shape) == 4 and s_ext.shape[1] == b_count)):
            raise HrxError(HRX_ERR_ARG, "s_ext: contiguous 64-bit limbs of shape [%d][s_pitch][4] or [%d][%d][s_pitch][4]" % (ncols, ncols, b_count))
        if selectors.dtype != u64 or not contiguous(selectors) or len(selectors.shape) != 3 or selectors.shape[0] != 3 or selectors.shape[2] != 4:
            raise HrxError(HRX_ERR_ARG, "selectors: contiguous 64-bit limbs of shape [3][sel_pitch][4]")
        cs = _theta_stride(beta, b_count, u64)
        if _theta_stride(gamma, b_count, u64) != cs or _theta_stride(y, b_count, u64) != cs:
            raise HrxError(HRX_ERR_ARG, "beta, gamma and y: all (4,) or all (%d, 4)" % b_count)
        for name, t in (("h_in", h_in), ("out", out)):
            if t is not None and (t.dtype != u64 or not contiguous(t) or len(t.shape) != 3 or t.shape[0] != b_count or t.shape[2] != 4):
                raise HrxError(HRX_ERR_ARG, "%s: contiguous 64-bit limbs of shape [%d][h_pitch][4]" % (name, b_count))
        if h_in is not None and out is not None and h_in.shape[1] != out.shape[1]:
            raise HrxError(HRX_ERR_ARG, "h_in and out: one h_pitch")
        if t_inv is not None and (t_inv.dtype != u64 or not contiguous(t_inv) or len(t_inv.shape) != 2 or t_inv.shape[1] != 4):
            raise HrxError(HRX_ERR_ARG, "t_inv: contiguous 64-bit limbs of shape [2^(ext_k - k)][4]")
        if out is None:
            out = _out_buffer(None, "out", (b_count, h_in.shape[1] if h_in is not None else max(1 << int(ext_k), 4), 4), u64, device, zeros=True)
        _check(call(b_count, pitch, s_ext.shape[-2], 1 if len(s_ext.shape) == 4 else 0, selectors.shape[1], cs, out, out.shape[1],
                    (FR_CANONICAL if canonical else 0) | (QUOTIENT_DIVIDE if divide else 0)))
        return out

    def lookup_quotient_selectors(self, k, ext_k, n_rows, shift, canonical=False, device=None, workspaces=None):
        """The selector columns lookup_quotient reads — l0 (the Lagrange basis polynomial of row 0), l_last (of row n_rows) and l_active (the sum of the bases
        of rows [0, n_rows)) — on the extended coset of generator `shift`, as limbs [3][2^ext_k][4]: three unit or indicator columns of 2^k rows through the
        existing transforms, inverse at k, then forward at ext_k with n_in = 2^k and the shift.  device None: numpy through fr_ntt_host (shift uint64 (4,));
        else torch through fr_ntt on that device (shift int64 CUDA limbs; workspaces: (fr_ntt_prepare(k), fr_ntt_prepare(ext_k)), prepared here where not
        given).  n_rows < 2^k.  Once per (k, ext_k, n_rows, shift)."""
        k, ext_k, n_rows = int(k), int(ext_k), int(n_rows)
        if not (1 <= k < ext_k <= 24) or not 0 <= n_rows < (1 << k):
            raise HrxError(HRX_ERR_ARG, "lookup_quotient_selectors: 1 <= k < ext_k <= 24, 0 <= n_rows < 2^k")
        n = 1 << k
        one = np.array(fr_from_u64(1, canonical), np.uint64)
        cols = np.zeros((3, max(n, 4), 4), np.uint64)
        cols[0, 0] = one
        cols[1, n_rows] = one
        cols[2, :n_rows] = one
        if device is None:
            coeff = self.fr_ntt_host(cols, k, inverse=True, n_in=n, canonical=canonical)
            return self.fr_ntt_host(coeff, ext_k, n_in=n, shift=shift, canonical=canonical)
        cols = torch.from_numpy(cols.view(np.int64)).to(device)
        ws_k, ws_ext = workspaces if workspaces is not None else (None, None)
        coeff = self.fr_ntt(cols, k, workspace=ws_k, inverse=True, n_in=n, canonical=canonical)
        return self.fr_ntt(coeff, ext_k, workspace=ws_ext, n_in=n, shift=shift, canonical=canonical)

    def witness_batch(self, chars, lens, out=None, stream=None):
        """Device-resident batch: chars (B, stride) uint8 CUDA tensor (stride % 16 == 0), lens (B,) int32 CUDA tensor.
        Asynchronous on `stream` (default: torch's current stream).  Returns (records, masked, status) tensors whose
        bit patterns are the u32/u16/u64 layouts of include/hrx.h."""
        assert chars.is_cuda and lens.is_cuda and chars.dtype == torch.uint8 and lens.dtype == torch.int32
        assert chars.stride(1) == 1 and lens.is_contiguous()
        B, stride = chars.shape[0], chars.stride(0)       # a (B, n) view of a wider buffer is fine
        if out is None:
            out = self.alloc_outputs(B, chars.device)
        rec, msk, st = out
        D = self.num_defs
        assert rec.stride(2) == 1 and rec.stride(1) == D and rec.stride(0) % D == 0 and msk.stride(1) == 1
        s = torch.cuda.current_stream(chars.device) if stream is None else stream
        _check(lib.hrx_witness_batch_device_pitched(self._need_device(chars, lens, rec, msk, st), chars.data_ptr(), stride, lens.data_ptr(), B,
                                                    self.max_chars_size, rec.data_ptr(), rec.stride(0) // D,
                                                    msk.data_ptr(), msk.stride(0), st.data_ptr(), s.cuda_stream))
        return rec, msk, st


# VERIFY (include/hrx.h): the check bits of a verdict word, the values tests/mock_prover.py gives them
VERIFY_FIRST_STATE, VERIFY_ENABLE, VERIFY_TRANSITION, VERIFY_START_LOOKUP, VERIFY_END_LOOKUP, VERIFY_ACCEPT = 1, 2, 4, 8, 16, 32
VERIFY_FLAGS, VERIFY_PADDING, VERIFY_MASK = 64, 128, 256
VERIFY_CIRCUIT_BITS = 63               # what MockProver::verify() itself sees
VERIFY_ROW_SHIFT = 32
VERIFY_NAMES = {VERIFY_FIRST_STATE: "first-state gate", VERIFY_ENABLE: "enable gate", VERIFY_TRANSITION: "transition lookup",
                VERIFY_START_LOOKUP: "start lookup", VERIFY_END_LOOKUP: "end lookup", VERIFY_ACCEPT: "accept chain",
                VERIFY_FLAGS: "flag completeness", VERIFY_PADDING: "padding", VERIFY_MASK: "masked rows"}


def verify_chunked_workspace_bytes(B, M, chunk_rows):
    """hrx_verify_chunked_workspace_bytes: the workspace of a chunked verify call; 0: chunk_rows is 0 or no multiple of 32"""
    return int(lib.hrx_verify_chunked_workspace_bytes(int(B), int(M), int(chunk_rows)))


def verdict_row(v):
    """the lowest row at which a reported check of verdict word v fails (0 when none does; None: the string is longer than max_chars_size and has no rows)"""
    v = int(v) & 0xffffffffffffffff
    return None if v == 0xffffffffffffffff else (v >> VERIFY_ROW_SHIFT) & 0x1ffffff


def explain_verdict(v):
    """a verdict word in words: "ok", or the failed checks and the lowest failing row"""
    v = int(v) & 0xffffffffffffffff
    if v == 0:
        return "ok"
    if v == 0xffffffffffffffff:
        return "longer than max_chars_size"
    return " + ".join(name for bit, name in VERIFY_NAMES.items() if v & bit) + " at row %d" % verdict_row(v)


def permuted_lookup_columns(n_table_rows, counts, n_rows):
    """The permuted columns of halo2's lookup argument out of one lookup's counts — no sort: index arrays (A_idx, S_idx) of length n_rows into the table rows.
    The n_rows - sum(counts) inputs not counted hit row 0 (rows outside the region evaluate to the dummy tuple) and the table is padded to n_rows with copies of
    row 0.  A_idx is non-decreasing with counts[t] copies of t (row 0: plus the uncounted inputs); S_idx is a permutation of the padded table; for every i,
    A_idx[i] == S_idx[i] or A_idx[i] == A_idx[i - 1].  ValueError: sum(counts) > n_rows or n_table_rows > n_rows."""
    m = np.asarray(counts, np.int64).copy()
    n_table_rows, n_rows = int(n_table_rows), int(n_rows)
    if m.ndim != 1 or len(m) != n_table_rows or n_table_rows < 1:
        raise ValueError("counts: one entry per table row")
    if n_table_rows > n_rows:
        raise ValueError("the table has more rows than the circuit")
    if int(m.sum()) > n_rows:
        raise ValueError("more counted inputs than the circuit has rows")
    m[0] += n_rows - int(m.sum())
    a_idx = np.repeat(np.arange(n_table_rows, dtype=np.int64), m)
    # the padded table as a multiset: row t once, row 0 another n_rows - n_table_rows times.  Where a run of A' begins, S' holds the run's row; the other
    # positions take what is left, in any order
    first = np.ones(n_rows, bool)
    first[1:] = a_idx[1:] != a_idx[:-1]
    s_idx = np.empty(n_rows, np.int64)
    s_idx[first] = a_idx[first]
    left = np.concatenate([np.nonzero(m == 0)[0], np.zeros(n_rows - n_table_rows, np.int64)])
    s_idx[~first] = left
    return a_idx, s_idx


FR_CANONICAL = 1                       # HRX_FR_CANONICAL
FR_COLUMN_NAMES = lambda D: (["char_enable", "characters"] + [n % d for d in range(D) for n in ("states[%d]", "substr_ids[%d]", "start_enable[%d]", "end_enable[%d]")]
                             + ["masked_characters", "all_substr_ids"])


FR_LOOKUP_COLUMN_NAMES = lambda D: [n % d for d in range(D) for n in ("trans[%d]", "start[%d]", "end[%d]")]      # hrx_lookup_compress_inputs_*


FR_NTT_INVERSE = 2                     # HRX_NTT_INVERSE
QUOTIENT_DIVIDE = 4                    # HRX_QUOTIENT_DIVIDE
FR_S = 28                              # bn256::Fr's two-adicity (halo2curves): r - 1 = 2^28 * odd, the multiplicative generator 7
FR_ROOT_OF_UNITY = 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c      # 7^((r - 1) / 2^28), of order exactly 2^28


def fr_sub(a, b):
    """hrx_fr_sub: a - b mod r of two elements given as 4 little-endian u64 limbs each (of one limb form); 4 limbs"""
    x, y, out = (C.c_uint64 * 4)(*[int(v) for v in a]), (C.c_uint64 * 4)(*[int(v) for v in b]), (C.c_uint64 * 4)()
    lib.hrx_fr_sub(x, y, out)
    return [int(v) for v in out]


def fr_mul(a, b):
    """hrx_fr_mul: the Montgomery product a * b / 2^256 mod r of two elements given as 4 little-endian u64 limbs each; 4 limbs"""
    x, y, out = (C.c_uint64 * 4)(*[int(v) for v in a]), (C.c_uint64 * 4)(*[int(v) for v in b]), (C.c_uint64 * 4)()
    lib.hrx_fr_mul(x, y, out)
    return [int(v) for v in out]


def fr_from_u64(v, canonical=False):
    """F::from(v) for F = bn256::Fr as the library computes it: 4 little-endian u64 limbs (Montgomery form unless canonical)."""
    out = (C.c_uint64 * 4)()
    lib.hrx_fr_from_u64(int(v), FR_CANONICAL if canonical else 0, out)
    return [int(x) for x in out]


class MultiDevice:
    """hrx_multi_*: one batch of host strings sharded by index over several devices (or several shards of one device), no
    collective.  MultiDevice(config, [0, 1, 2, 3]).witness_batch_host(chars, lens) == config.witness_batch_host(chars, lens)."""

    def __init__(self, config, devices):
        self._cfg = config
        self._h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        _check(lib.hrx_multi_create(config._defs.h, arr, len(devices), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            lib.hrx_multi_destroy(self._h)
            self._h = None

    @property
    def num_shards(self):
        return lib.hrx_multi_num_shards(self._h)

    def shard_device(self, shard):
        return lib.hrx_multi_shard_device(self._h, shard)

    def witness_batch_device(self, shards, layout=LAYOUT_POSITION_MAJOR | LAYOUT_INPUT_POSITION_MAJOR, chars_stride=None):
        """hrx_multi_witness_batch_device: `shards` = one (chars, lens, (records, masked, status)) per shard, CUDA tensors on
        that shard's device (outputs as made by alloc_outputs_position_major / alloc_outputs on that device).  Asynchronous:
        one kernel per shard on the shard's own stream; synchronize() waits for all.  No PCIe traffic, no collective.
        Every shard's stream first waits for what torch's current stream of that device has been given so far (the kernels
        that produced the inputs).  chars_stride: the per-string capacity in bytes; required for flat position-major
        inputs unless it follows from the buffer sizes (numel(chars) / numel(lens), the same for every shard)."""
        n = self.num_shards
        assert len(shards) == n
        vpa, sza = C.c_void_p * n, C.c_size_t * n
        chars, lens, recs, msks, sts, counts = vpa(), vpa(), vpa(), vpa(), vpa(), sza()
        strides = set()
        for r, (c, l, (rec, msk, st)) in enumerate(shards):
            for t in (c, l, rec, msk, st):
                if t.numel() and t.device.index != self.shard_device(r):
                    raise HrxError(HRX_ERR_ARG, "shard %d: tensor on %s, shard lives on cuda:%d" % (r, t.device, self.shard_device(r)))
            chars[r], lens[r], recs[r], msks[r], sts[r], counts[r] = c.data_ptr(), l.data_ptr(), rec.data_ptr(), msk.data_ptr(), st.data_ptr(), l.numel()
            if chars_stride is None and l.numel():
                if c.dim() == 2 and not (layout & LAYOUT_INPUT_POSITION_MAJOR):
                    strides.add(int(c.stride(0)))
                elif c.numel() % l.numel() == 0:
                    strides.add(c.numel() // l.numel())
                else:
                    raise HrxError(HRX_ERR_ARG, "shard %d: chars_stride not given and numel(chars) is not a multiple of numel(lens)" % r)
        if chars_stride is not None:
            stride = int(chars_stride)
        elif len(strides) == 1:
            stride = strides.pop()
        elif not strides:
            stride = 16      # every shard is empty: nothing is launched
        else:
            raise HrxError(HRX_ERR_ARG, "chars_stride not given and the shards' buffers imply different strides: %s" % sorted(strides))
        if stride % 16 or stride < 16:
            raise HrxError(HRX_ERR_ARG, "chars stride %d: must be a multiple of 16 bytes, >= 16" % stride)
        for r in range(n):     # order each shard's private stream behind the producer of its inputs
            if counts[r]:
                d = self.shard_device(r)
                torch.cuda.ExternalStream(lib.hrx_multi_shard_stream(self._h, r), device=torch.device("cuda", d)).wait_stream(torch.cuda.current_stream(d))
        _check(lib.hrx_multi_witness_batch_device(self._h, layout, chars, stride, lens, counts, self._cfg.max_chars_size, recs, msks, sts))

    def synchronize(self):
        _check(lib.hrx_multi_synchronize(self._h))

    def witness_batch_host(self, chars2d, lens, out=None):
        chars2d = _np(chars2d, np.uint8)
        lens = _np(lens, np.uint32)
        B, stride = chars2d.shape
        M, D = self._cfg.max_chars_size, self._cfg.num_defs
        if out is None:
            out = np.zeros((B, M, D), np.uint32), np.zeros((B, M), np.uint16), np.zeros(B, np.uint64)
        rec, msk, st = out
        _check(lib.hrx_multi_witness_batch_host(self._h, _ptr(chars2d, _u8p), stride, _ptr(lens, _u32p), B, M,
                                                _ptr(rec, _u32p), _ptr(msk, _u16p), _ptr(st, _u64p)))
        return rec, msk, st


def decode_spans(counts, spans):
    """(counts (B,), spans (B, max_spans)) of a match call -> per string a list of (substr_id, start, length), the first
    min(count, max_spans) runs (include/hrx.h: bits 0..27 start, 28..55 length, 56..63 masked_substr_id)."""
    counts = counts.cpu().numpy() if hasattr(counts, "cpu") else np.asarray(counts)
    spans = spans.cpu().numpy() if hasattr(spans, "cpu") else np.asarray(spans)
    spans = spans.view(np.uint64) if spans.dtype != np.uint64 else spans
    out = []
    for b in range(len(counts)):
        k = min(int(counts[b]) & 0xFFFFFFFF, spans.shape[1] if spans.ndim == 2 else 0)
        row = []
        for w in spans[b, :k]:
            w = int(w)
            row.append((w >> 56, w & 0xFFFFFFF, (w >> 28) & 0xFFFFFFF))
        out.append(row)
    return out


def runs_from_masked(masked, lens, status):
    """The runs a match call reports, from witness output: masked rows (B, M) u16 -> (counts, per string [(substr_id, start, length)]), the maximal
    runs of one non-zero masked_substr_id (masked >> 8) below n_b; none where the status code != 0."""
    masked, lens, status = np.asarray(masked), np.asarray(lens), np.asarray(status)
    counts, runs = [], []
    for b in range(masked.shape[0]):
        r = []
        if not int(status[b]) & 0xff:
            v = masked[b].astype(np.int64) >> 8
            v[int(lens[b]):] = 0
            cuts = np.flatnonzero(np.diff(v)) + 1
            starts, ends = np.concatenate(([0], cuts)), np.concatenate((cuts, [len(v)]))
            r = [(int(v[s]), int(s), int(e - s)) for s, e in zip(starts, ends) if v[s] != 0]
        counts.append(len(r))
        runs.append(r)
    return counts, runs


def revealed_substrings(chars, lens, status, counts, spans):
    """Per string a list of (substr_id, start, bytes) — what the circuit reveals (lib.rs:1046-1058); [] for strings whose status code != 0.
    chars: (B, stride) string-major bytes (numpy or tensor)."""
    chars = chars.cpu().numpy() if hasattr(chars, "cpu") else np.asarray(chars)
    status = status.cpu().numpy() if hasattr(status, "cpu") else np.asarray(status)
    res = []
    for b, runs in enumerate(decode_spans(counts, spans)):
        if int(status[b]) & 0xff:
            res.append([])
            continue
        res.append([(sid, start, bytes(chars[b, start:start + length])) for sid, start, length in runs])
    return res


def pack_strings(strings):
    """A list of bytes -> (values uint8, offsets uint64 (B + 1)): the strings back to back (an Arrow large-binary column), values padded with
    zeros to a multiple of 16 bytes (the device entry points read whole aligned 16-byte chunks)."""
    lens = np.fromiter((len(x) for x in strings), dtype=np.uint64, count=len(strings))
    offsets = np.zeros(len(strings) + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    total = int(offsets[-1])
    values = np.zeros(-(-total // 16) * 16, np.uint8)
    if total:
        values[:total] = np.frombuffer(b"".join(bytes(x) for x in strings), np.uint8)
    return values, offsets


def revealed_substrings_ragged(values, offsets, status, counts, spans):
    """revealed_substrings for a ragged batch: per string a list of (substr_id, start, bytes); [] where the status code != 0."""
    values = values.cpu().numpy() if hasattr(values, "cpu") else np.asarray(values)
    offsets = offsets.cpu().numpy() if hasattr(offsets, "cpu") else np.asarray(offsets)
    status = status.cpu().numpy() if hasattr(status, "cpu") else np.asarray(status)
    offsets = offsets.astype(np.uint64)
    res = []
    for b, runs in enumerate(decode_spans(counts, spans)):
        if int(status[b]) & 0xff:
            res.append([])
            continue
        o = int(offsets[b])
        res.append([(sid, start, bytes(values[o + start:o + start + length])) for sid, start, length in runs])
    return res


#: what the extract calls return (include/hrx.h EXTRACT): the match call's status / counts and the list column — torch tensors (int64 / int32 / uint8 holding the
#: u64 / u32 / u8 words) from the device forms, numpy arrays from the host forms
Extracted = collections.namedtuple("Extracted", "status counts run_offsets runs byte_offsets values totals")


def extract_workspace_bytes(B):
    return lib.hrx_extract_workspace_bytes(int(B))


def extract_spans_host(src, status, counts, spans, offsets=None, require_accept=0, caps=None, out=None, threads=0):
    """hrx_extract_spans_host (no context): src = chars (B, stride) uint8, or ragged values with offsets (B + 1) uint64; status / counts / spans: the outputs of
    a match call on it.  caps = (runs_cap, values_cap), default B * max_spans and the input's byte count; out = (run_offsets, runs, byte_offsets, values,
    totals): the caller's arrays (their sizes are the caps then).  -> Extracted of numpy arrays."""
    src = _np(src, np.uint8)
    status, counts, spans = _np(status, np.uint64), _np(counts, np.uint32), _np(spans, np.uint64)
    B, max_spans = len(status), spans.shape[1]
    if offsets is not None:
        offsets = _np(offsets, np.uint64)
        layout, stride = LAYOUT_INPUT_RAGGED, 0
    else:
        layout, stride = LAYOUT_STRING_MAJOR, src.shape[1]
    if out is None:
        runs_cap, values_cap = caps or (B * max_spans, src.size)
        out = (np.zeros(B + 1, np.uint64), np.zeros(runs_cap, np.uint64), np.zeros(runs_cap + 1, np.uint64), np.zeros(values_cap, np.uint8), np.zeros(4, np.uint64))
    ro, runs, bo, vals, tot = out
    assert len(ro) == B + 1 and len(bo) == len(runs) + 1 and len(tot) == 4
    o = _ExtractOutC(ro.ctypes.data, runs.ctypes.data, bo.ctypes.data, vals.ctypes.data, tot.ctypes.data, len(runs), len(vals))
    _check(lib.hrx_extract_spans_host(layout, src.ctypes.data, stride, offsets.ctypes.data if offsets is not None else None, B, status.ctypes.data,
                                      counts.ctypes.data, spans.ctypes.data, max_spans, int(require_accept), C.byref(o), int(threads)))
    return Extracted(status, counts, ro, runs, bo, vals, tot)


#: what route / route_host return (include/hrx.h ROUTE): bucket j is order[bucket_offsets[j]:bucket_offsets[j + 1]], range n_buckets the strings not kept
Routed = collections.namedtuple("Routed", "order bucket_offsets")
MAX_BUCKETS = 8                      # HRX_MAX_BUCKETS


def route_workspace_bytes(B):
    return lib.hrx_route_workspace_bytes(int(B))


def route_host(status, lens=None, offsets=None, bounds=None, require_accept=0, out=None):
    """hrx_route_host (no context): status (B,) uint64 of a match call or None, lens (B,) uint32 or ragged offsets (B + 1,) uint64 (exactly one), bounds: the
    circuit sizes (required here: there is no config to take a default from); out = (order uint32 (B,), bucket_offsets uint64 (n_buckets + 2,)): the
    caller's arrays.  -> Routed of numpy arrays."""
    bounds = _np([] if bounds is None else bounds, np.uint32)
    status = None if status is None else _np(status, np.uint64)
    lens = None if lens is None else _np(lens, np.uint32)
    offsets = None if offsets is None else _np(offsets, np.uint64)
    if lens is not None:
        B = len(lens)
    elif offsets is not None:
        B = len(offsets) - 1
    else:
        B = 0 if status is None else len(status)
    assert B >= 0 and (status is None or len(status) == B)
    if out is None:
        out = np.zeros(B, np.uint32), np.zeros(len(bounds) + 2, np.uint64)
    order, bo = out
    assert len(order) == B and len(bo) == len(bounds) + 2 and order.dtype == np.uint32 and bo.dtype == np.uint64
    _check(lib.hrx_route_host(status.ctypes.data if status is not None else None, int(require_accept), lens.ctypes.data if lens is not None else None,
                              offsets.ctypes.data if offsets is not None else None, B, _ptr(bounds, _u32p), len(bounds), order.ctypes.data, bo.ctypes.data))
    return Routed(order, bo)


def _extracted_host(ex):
    """the arrays of an Extracted on the host as unsigned numpy; raises where the caps were too small (totals says what is needed)"""
    a = [x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in ex]
    st, cnt, ro, runs, bo, vals, tot = [x.view(dt) if x.dtype != dt else x for x, dt in zip(a, (np.uint64, np.uint32, np.uint64, np.uint64, np.uint64, np.uint8, np.uint64))]
    R, nbytes = int(tot[0]), int(tot[1])
    if R > len(runs) or nbytes > len(vals):
        raise ValueError("extract: %d runs / %d bytes needed, caps %d / %d" % (R, nbytes, len(runs), len(vals)))
    return ro, runs[:R], bo[:R + 1], vals[:nbytes]


def extracted_lists(ex):
    """An Extracted -> per string a list of (substr_id, start, bytes): the shape revealed_substrings returns, so the two compare directly."""
    ro, runs, bo, vals = _extracted_host(ex)
    raw = vals.tobytes()
    res = []
    for b in range(len(ro) - 1):
        row = []
        for j in range(int(ro[b]), int(ro[b + 1])):
            w = int(runs[j])
            row.append((w >> 56, w & 0xFFFFFFF, raw[int(bo[j]):int(bo[j + 1])]))
        res.append(row)
    return res


def extracted_column(ex, substr_id):
    """An Extracted -> (values uint8, offsets uint64 (B + 1)): per string the concatenation of its runs with this masked_substr_id, back to back — the
    large-binary column an indexer stores for one public part."""
    ro, runs, bo, vals = _extracted_host(ex)
    B = len(ro) - 1
    keep = (runs >> np.uint64(56)) == np.uint64(substr_id)
    lens = np.where(keep, bo[1:] - bo[:-1], np.uint64(0)).astype(np.uint64)
    csum = np.concatenate((np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)))
    offsets = csum[ro.astype(np.int64)]                     # bytes of this id in front of each string's first run
    pick = np.repeat(keep, (bo[1:] - bo[:-1]).astype(np.int64))
    assert len(offsets) == B + 1
    return vals[pick], offsets


def decode_status(s):
    s = int(s) & 0xFFFFFFFFFFFFFFFF
    code = s & 0xff
    if code == 0:
        return {"code": 0, "accept": (s >> 8) & 0xffffffff}
    if code == 1:
        return {"code": 1, "def": (s >> 8) & 0xff, "char": (s >> 16) & 0xff, "state": (s >> 24) & 0xffff, "pos": s >> 40}
    if code == 2:
        return {"code": 2, "pos": s >> 40}
    return {"code": code}
