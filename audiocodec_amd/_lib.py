"""ctypes binding of ``libaudiocodec_amd.so`` (the C ABI declared in ``include/audiocodec_amd.h``).

There is no fallback: if the shared library is missing or a call fails the product raises.
"""

from __future__ import annotations

import ctypes
import os
import threading
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AUDIOCODEC_AMD_LIB") or os.path.join(_HERE, "lib", "libaudiocodec_amd.so")

AC_OK = 0
AC_EINVAL, AC_EHIP, AC_ENOMEM, AC_ENODEV, AC_EUNSUPPORTED = -1, -2, -3, -4, -5
AC_EMIT_NOISY, AC_EMIT_DB_NORM, AC_EMIT_CODES, AC_EMIT_PACKED = 1, 2, 4, 8   # flags of ac_encode_fused_ex
AC_PACKED = 16   # spectrum-side format of ac_stream_encode_typed / ac_stream_inverse_typed: packed rows
AC_IN_PCM16 = 32   # x is int16 PCM: flag of ac_encode_fused_ex beside AC_EMIT_CODES / AC_EMIT_PACKED, and of
                   # ac_stream_encode_typed's dtype beside AC_PACKED
AC_IN_PACKED = 64  # x is one ac_packed_rows: flag of ac_encode_fused_ex beside AC_EMIT_PACKED alone (transrating)
AC_EMIT_REDUNDANT = 256   # beside AC_IN_PACKED | AC_EMIT_PACKED: out0 is one ac_protected_out (protected slots)
AC_EMIT_CARRY = 512   # beside the three flags of protecting: the rows are a chunk of a stream, out1 is one ac_protect_carry
AC_IN_MIX = 1024   # beside AC_IN_PACKED | AC_EMIT_PACKED: x is one ac_mix_rows (the rows of several sources mixed)
AC_MIX_MAX_SOURCES = 8   # the most sources the one launch of AC_IN_MIX reads (the header's macro)
AC_IN_ROUTE = 2048   # beside AC_IN_PACKED | AC_EMIT_PACKED: x is one ac_route_rows (the rows of several sources to several mixes)
AC_ROUTE_MAX_SOURCES = 4   # the most sources and ...
AC_ROUTE_MAX_OUTPUTS = 8   # ... outputs the one launch of AC_IN_ROUTE serves (the header's macros)
AC_ROUTE_MUTE = -32768   # in ac_route_rows' gain: the output does not hear the source (the header's macro)
AC_EMIT_LEVEL = 4096   # beside AC_IN_PACKED alone: out0 is float energy, out1 NULL or uint8 bad (the level of packed rows)
AC_SELECT_ACTIVE = 8192   # alone: x is one ac_select_rows, out0 uint8 active (the n loudest sources)
AC_SELECT_MAX_SOURCES = 64   # the most sources AC_SELECT_ACTIVE ranks (the header's macro)
AC_CONCEAL_REDUNDANT = 256   # in ac_conceal's max_age: the struct is an ac_conceal_redundant (lost rows recovered)
AC_CONCEAL = 128   # beside AC_PACKED in ac_stream_inverse_typed's dtype: X_chunk is one ac_stream_packed_lost_in
AC_PACK_ROWS_MAX_BITS = 16384 # the largest row budget AC_EMIT_PACKED serves in one launch (the header's macro)
AC_CONCEAL_FADE = 4       # scale-factor units a concealed row loses per frame of age (the header's macro)
AC_CONCEAL_MAX_AGE = 31   # the largest max_age of ac_conceal (the header's macro)
WINDOW_IDS = {"vorbis": 0, "sine": 1}   # anything else -> 2 (rectangular), mdctransformer.py:199-211
WINDOW_RECT = 2

# name -> (restype, argtypes); mirrors include/audiocodec_amd.h (+ the test hook of audiocodec_amd_testing.h) one to one
PROTOTYPES = {
    "ac_version": (c_int, []),
    "ac_last_error": (c_char_p, []),
    "ac_set_force_generic": (c_int, [c_int]),
    "ac_testing_runs_image": (c_int, [c_int, c_int, c_double, c_double, c_int, POINTER(ctypes.c_uint32), c_int, POINTER(c_int)]),
    "ac_mdct_fold_coefficients_host": (c_int, [c_int, c_int, POINTER(c_double)]),
    "ac_mdct_dense_matrices_host": (c_int, [c_int, c_int, POINTER(c_float), POINTER(c_float)]),
    "ac_psy_tables_host": (c_int, [c_int, c_int, c_double, c_double, POINTER(c_float), POINTER(c_float),
                                   POINTER(c_float), POINTER(c_float), POINTER(c_double)]),
    "ac_psy_tables_host_f64": (c_int, [c_int, c_int, c_double, c_double, POINTER(c_double), POINTER(c_double),
                                       POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "ac_mdct_fold_coefficients_host_pre": (c_int, [c_int, c_int, c_int, POINTER(c_double)]),
    "ac_mdct_dense_matrices_host_pre": (c_int, [c_int, c_int, c_int, POINTER(c_float), POINTER(c_float)]),
    "ac_psy_tables_host_pre": (c_int, [c_int, c_int, c_double, c_double, c_int, POINTER(c_double), POINTER(c_double),
                                       POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "ac_mdct_plan_create_pre": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "ac_psy_plan_create_pre": (c_int, [c_int, c_int, c_double, c_double, c_int, c_int, c_int, POINTER(c_void_p)]),
    "ac_mdct_plan_adjoint": (c_int, [c_void_p, POINTER(c_void_p)]),
    "ac_mdct_plan_create": (c_int, [c_int, c_int, c_int, POINTER(c_void_p)]),
    "ac_mdct_plan_destroy": (c_int, [c_void_p]),
    "ac_psy_plan_create": (c_int, [c_int, c_int, c_double, c_double, c_int, POINTER(c_void_p)]),
    "ac_psy_plan_destroy": (c_int, [c_void_p]),
    "ac_mdct_plan_is_fast": (c_int, [c_void_p]),
    "ac_mdct_plan_tier": (c_int, [c_void_p, c_int]),
    "ac_psy_plan_is_fast": (c_int, [c_void_p]),
    "ac_psy_plan_tier": (c_int, [c_void_p]),
    "ac_psy_plan_create_ex": (c_int, [c_int, c_int, c_double, c_double, c_int, c_int, POINTER(c_void_p)]),
    "ac_psy_plan_spreading": (c_int, [c_void_p]),
    "ac_mdct_forward_typed": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ac_mdct_inverse_typed": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ac_tonality_typed": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ac_mask_threshold_typed": (c_int, [c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_int, c_int, c_int, c_int,
                                        c_void_p]),
    "ac_tonality_backward_typed": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ac_mask_threshold_backward_typed": (c_int, [c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                                 c_int, c_void_p]),
    "ac_workspace_create": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_double, c_void_p, POINTER(c_void_p)]),
    "ac_workspace_buffers": (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                                     POINTER(c_void_p)]),
    "ac_workspace_regions": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_size_t), POINTER(c_void_p), POINTER(c_size_t)]),
    "ac_workspace_report": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_float), POINTER(c_double)]),
    "ac_workspace_destroy": (c_int, [c_void_p]),
    "ac_workspace_alloc_dlpack": (c_void_p, [c_void_p, c_int, c_int, POINTER(ctypes.c_int64), c_void_p]),
    "ac_workspace_live": (ctypes.c_long, [c_void_p]),
    "ac_workspace_record_stream": (c_int, [c_void_p, c_void_p, c_void_p]),
    "ac_probe_placement": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p), c_int, c_int, c_int,
                                   c_int, c_void_p, POINTER(c_int), POINTER(c_float)]),
    "ac_encode_fused_typed": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_int, c_int,
                                      c_int, c_int, c_void_p]),
    "ac_stream_encode_typed": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_int, c_int, c_void_p]),
    "ac_stream_inverse_typed": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "ac_amplitude_to_db_typed": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    "ac_add_noise_typed": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_uint64, c_int, c_void_p]),
    "ac_mdct_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ac_mdct_inverse": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ac_tonality": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ac_mask_threshold": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ac_tonality_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ac_mask_threshold_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int,
                                           c_int, c_int, c_void_p]),
    "ac_encode_launches": (c_int, [c_void_p, c_void_p, c_int]),
    "ac_encode_fused": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int,
                                c_int, c_void_p]),
    "ac_encode_fused_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p,
                                   c_void_p, c_uint64, c_int, c_int, c_int, c_void_p]),
    "ac_amplitude_to_db_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "ac_mdct_forward_pcm16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ac_mdct_inverse_pcm16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ac_encode_fused_pcm16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int,
                                      c_int, c_int, c_void_p]),
    "ac_stream_create": (c_int, [c_void_p, c_int, c_int, POINTER(c_void_p)]),
    "ac_stream_reset": (c_int, [c_void_p, c_void_p]),
    "ac_stream_destroy": (c_int, [c_void_p]),
    "ac_stream_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "ac_stream_inverse": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "ac_stream_settle": (c_int, [c_void_p, c_void_p]),
    "ac_stream_run": (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                              POINTER(c_void_p), POINTER(c_void_p), c_float, c_void_p]),
    "ac_stream_encode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "ac_amplitude_to_db": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "ac_add_noise": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_uint64, c_void_p]),
    "ac_psy_scale_bands_host": (c_int, [c_double, c_int, c_int, POINTER(ctypes.c_int32)]),
    "ac_quantize": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ac_dequantize": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ac_decode_quantized": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                    c_void_p]),
    "ac_decode_quantized_launches": (c_int, [c_void_p, c_void_p, c_int]),
    "ac_encode_quantized_launches": (c_int, [c_void_p, c_void_p, c_int]),
    "ac_decode_packed_launches": (c_int, [c_void_p, c_void_p, c_int]),
    "ac_encode_packed_launches": (c_int, [c_void_p, c_void_p, c_int]),
    "ac_stream_packed_launches": (c_int, [c_void_p, c_void_p, c_int]),
    "ac_encode_quantized_launches_pcm16": (c_int, [c_void_p, c_void_p, c_int]),
    "ac_encode_packed_launches_pcm16": (c_int, [c_void_p, c_void_p, c_int]),
    "ac_stream_packed_launches_pcm16": (c_int, [c_void_p, c_void_p]),
    "ac_transrate_launches": (c_int, [c_void_p, c_int]),
    "ac_mix_launches": (c_int, [c_void_p, c_int, c_int]),
    "ac_route_launches": (c_int, [c_void_p, c_int, c_int, c_int]),
    "ac_level_launches": (c_int, [c_void_p, c_int]),
    "ac_protect_launches": (c_int, [c_void_p, c_int, c_int]),
    "ac_protect_chunk_launches": (c_int, [c_void_p, c_int, c_int]),
    "ac_pack_scratch_bytes": (c_size_t, [c_int, c_int, c_int]),
    "ac_pack_index": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ac_pack": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ac_unpack": (c_int, [c_void_p, c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ac_quantize_budget": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int, c_int, c_int, c_void_p]),
    "ac_psy_plan_with_row_budget": (c_int, [c_void_p, c_int, c_int, POINTER(c_void_p)]),
    "ac_psy_plan_row_budget": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "ac_clip_budget_scratch_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "ac_quantize_clip_budget": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_void_p, c_int, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
}

class PackedRows(ctypes.Structure):
    """``ac_packed_rows``: what ``ac_decode_quantized`` takes for ``codes`` when ``sf`` is NULL."""
    _fields_ = [("data", c_void_p), ("nbytes", ctypes.c_int64), ("index", c_void_p)]


class MixRows(ctypes.Structure):
    """``ac_mix_rows``: what ``ac_encode_fused_ex`` takes for ``x`` under ``AC_IN_MIX``."""
    _fields_ = [("sources_n", ctypes.c_int32), ("src", POINTER(PackedRows)), ("gain", POINTER(ctypes.c_int32)), ("active", c_void_p)]


class RouteRows(ctypes.Structure):
    """``ac_route_rows``: what ``ac_encode_fused_ex`` takes for ``x`` under ``AC_IN_ROUTE``."""
    _fields_ = [("sources_n", ctypes.c_int32), ("outputs_n", ctypes.c_int32), ("src", POINTER(PackedRows)),
                ("gain", POINTER(ctypes.c_int32)), ("active", c_void_p)]


class SelectRows(ctypes.Structure):
    """``ac_select_rows``: what ``ac_encode_fused_ex`` takes for ``x`` under ``AC_SELECT_ACTIVE``."""
    _fields_ = [("sources_n", ctypes.c_int32), ("energy", c_void_p), ("valid", c_void_p), ("n", ctypes.c_int32),
                ("release", c_float), ("gate", c_float), ("state", c_void_p)]


class Conceal(ctypes.Structure):
    """``ac_conceal``: what ``ac_decode_quantized`` takes for ``scratch`` when ``sf`` is NULL (lost rows concealed)."""
    _fields_ = [("lost", c_void_p), ("max_age", ctypes.c_int32)]


class ConcealRedundant(ctypes.Structure):
    """``ac_conceal_redundant``: ``ac_conceal`` with ``AC_CONCEAL_REDUNDANT`` in ``max_age``, then where the copies lie."""
    _fields_ = [("lost", c_void_p), ("max_age", ctypes.c_int32), ("redundant_at", ctypes.c_int64)]


class ProtectedOut(ctypes.Structure):
    """``ac_protected_out``: what ``ac_encode_fused_ex`` takes for ``out0`` under ``AC_EMIT_REDUNDANT``."""
    _fields_ = [("data", c_void_p), ("row_bytes", ctypes.c_int64), ("fits", c_void_p), ("red_bits", ctypes.c_int32),
                ("red_fits", c_void_p), ("offset", c_void_p), ("red_offset", c_void_p)]


class PackedOut(ctypes.Structure):
    """``ac_packed_out``: what ``ac_encode_fused_ex`` takes for ``out0`` under ``AC_EMIT_PACKED``."""
    _fields_ = [("data", c_void_p), ("row_bytes", ctypes.c_int64), ("fits", c_void_p)]


class QuantizedRows(ctypes.Structure):
    """``ac_quantized_rows``: what ``ac_quantize_budget`` takes for ``X`` when ``thr`` is NULL (the requantiser)."""
    _fields_ = [("codes", c_void_p), ("sf", c_void_p)]


class ProtectCarry(ctypes.Structure):
    """``ac_protect_carry``: what ``ac_encode_fused_ex`` takes for ``out1`` under ``AC_EMIT_CARRY``."""
    _fields_ = [("row_in", c_void_p), ("fits_in", c_void_p), ("offset_in", c_void_p), ("row_out", c_void_p), ("fits_out", c_void_p),
                ("offset_out", c_void_p)]


class StreamPackedIn(ctypes.Structure):
    """``ac_stream_packed_in``: what ``ac_stream_inverse_typed`` takes for ``X_chunk`` under ``AC_PACKED``."""
    _fields_ = [("rows", PackedRows), ("psy", c_void_p), ("pcm16", ctypes.c_int32)]


class StreamPackedLostIn(ctypes.Structure):
    """``ac_stream_packed_lost_in``: what ``ac_stream_inverse_typed`` takes for ``X_chunk`` under ``AC_PACKED | AC_CONCEAL``."""
    _fields_ = [("inner", StreamPackedIn), ("lost", c_void_p), ("max_age", ctypes.c_int32)]


class StreamPackedRecoverIn(ctypes.Structure):
    """``ac_stream_packed_recover_in``: ``ac_stream_packed_lost_in`` with ``AC_CONCEAL_REDUNDANT`` in ``max_age``, then where
    the copies lie -- a recovering chunk, one frame behind its rows."""
    _fields_ = [("inner", StreamPackedIn), ("lost", c_void_p), ("max_age", ctypes.c_int32), ("redundant_at", ctypes.c_int64)]


_lock = threading.Lock()
_lib = None


class AudioCodecError(RuntimeError):
    """A libaudiocodec_amd call returned a non-zero status."""

    def __init__(self, status, message):
        super().__init__("libaudiocodec_amd status %d: %s" % (status, message))
        self.status = status


def load():
    """Load (once) and return the ctypes handle.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH) and not os.environ.get("AUDIOCODEC_AMD_LIB"):
            _build_in_tree()
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C audiocodec_amd/csrc`.  There is no CPU fallback.%s"
                % (LIB_PATH, ("\n--- output of the in-tree build attempt ---\n" + _build_log) if _build_log else ""))
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(lib, name)          # AttributeError here = header/library mismatch
            fn.restype = restype
            fn.argtypes = argtypes
        if lib.ac_version() < 171:
            raise ImportError("libaudiocodec_amd too old: %d" % lib.ac_version())
        _lib = lib
    return _lib


_build_log = ""


def _build_in_tree():
    """The library is built in-tree by ``__graft_entry__.build()`` / ``make -C audiocodec_amd/csrc``; when it is missing
    (a fresh checkout) try that once -- hipcc cross-compiles for gfx950 without a GPU.  Ranks importing at the same time
    serialise on a file lock; the build links into a scratch directory and renames the library into place, so nobody can
    dlopen a half-written file.  A failure is not hidden: load() raises ImportError with the compiler's output."""
    global _build_log
    import fcntl
    import shutil
    import subprocess
    import tempfile
    # under a profiler (rocprofv3 preloads a library that initialises the GPU in every child) the make / hipcc / clang
    # children would exec from GPU-initialised processes, which this pool forbids: refuse, do not build
    preload = [k for k in os.environ if k.startswith(("ROCP", "ROCPROFILER", "ROCTRACER"))]
    if preload or "rocprof" in os.environ.get("LD_PRELOAD", ""):
        _build_log = ("not building under a profiler (%s set): run `make -C audiocodec_amd/csrc` (or __graft_entry__.build()) "
                      "before the profiled command" % ", ".join(preload or ["LD_PRELOAD"]))
        return
    libdir = os.path.join(_HERE, "lib")
    os.makedirs(libdir, exist_ok=True)
    with open(os.path.join(libdir, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if os.path.exists(LIB_PATH):          # another process built it while this one waited
                return
            tmp = tempfile.mkdtemp(prefix="build_", dir=libdir)
            try:
                r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j4", "OUTDIR=" + tmp],
                                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
                _build_log = r.stdout[-4000:]
                if r.returncode == 0:
                    os.replace(os.path.join(tmp, "libaudiocodec_amd.so"), LIB_PATH)
            except (OSError, subprocess.SubprocessError) as e:
                _build_log = "%s: %s" % (type(e).__name__, e)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def check(status):
    """Turn a non-zero status into an exception (ValueError for AC_EINVAL, like a shape error)."""
    if status == AC_OK:
        return
    msg = load().ac_last_error()
    msg = msg.decode("utf-8", "replace") if msg else ""
    if status == AC_EINVAL:
        raise ValueError(msg)
    raise AudioCodecError(status, msg)


def window_id(window_type):
    """Reference semantics (mdctransformer.py:199-211): case-insensitive 'sine' / 'vorbis', else rectangular.
    ``None`` selects the rectangular window (the reference raises AttributeError; documented fix)."""
    if isinstance(window_type, str):
        return WINDOW_IDS.get(window_type.lower(), WINDOW_RECT)
    if window_type is None:
        return WINDOW_RECT
    raise TypeError("window_type must be a string or None")
