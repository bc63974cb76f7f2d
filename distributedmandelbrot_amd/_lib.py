"""ctypes binding of libmbk_hip.so (C ABI: include/mbk.h).

The library is built in-tree by ``distributedmandelbrot_amd.build`` and loaded from this directory.
If it is missing the import of the product path FAILS LOUDLY -- there is no CPU fallback
(the CPU oracle under oracle/ is test infrastructure and is never imported from here).
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(HERE, "libmbk_hip.so")

MBK_OK, MBK_ERR_INVALID, MBK_ERR_NO_DEVICE, MBK_ERR_HIP, MBK_ERR_NOMEM, MBK_ERR_NET = range(6)
MBK_WANT_COUNTS = 0x1
MBK_WANT_BYTES = 0x2
MBK_KERNEL_DEFAULT = 0x000
MBK_KERNEL_SIMPLE = 0x100
MBK_KERNEL_ASM = 0x200
MBK_KERNEL_REFILL = 0x300
MBK_KERNEL_GROUP = 0x400
MBK_KERNEL_SCAN = 0x500
KERNELS = {"default": MBK_KERNEL_DEFAULT, "simple": MBK_KERNEL_SIMPLE, "asm": MBK_KERNEL_ASM,
           "refill": MBK_KERNEL_REFILL, "group": MBK_KERNEL_GROUP, "scan": MBK_KERNEL_SCAN}
# enum mbk_option (include/mbk.h), in order
OPTIONS = {name: i for i, name in enumerate(
    ["order", "waves_per_wg", "group_steps", "exact_steps", "probe_steps", "scan_waves", "scan_xcd_map", "scan_col_period", "heavy_share",
     "rf_livemin", "rf_patience", "rf_batch", "rf_waves", "cycle_detect", "probe_mid", "prepass_overlap", "exact_long", "scan_inline", "wave_limit", "units_min_light", "xcd_balance", "m_late", "h_settled", "classify_wg", "scan_strip", "cycle_window", "spill_first", "spill_lanes", "spill_min_mrd", "spill_min_blocks", "spill_cyc_shift",
     "sure_interior"])}
MBK_PRECISION_F32 = 0x1000
MBK_LAZY_UNIFORM = 0x2000
MBK_DEEP_BLA = 0x8000   # deep count / render / histogram calls only
MBK_DEEP_XBLA = 0x10000   # extended-range deep count / render / histogram calls only
PRECISIONS = {"f64": 0, "f32": MBK_PRECISION_F32}
MBK_SLOTS = 4
MBK_WORKER_DEPTH = 3
MBK_INFO_SCAN_WG_PER_CU = 100
MBK_INFO_XCD_SHARE = 110
MBK_INFO_SPILL = 130
MBK_CODEC_RAW = 0x00
MBK_CODEC_RLE = 0x01
MBK_CHUNK_DEFINITION = 4096
MBK_CHUNK_BYTES = 4096 * 4096
MBK_ABI_VERSION = 5
MBK_RENDER_BYTES = 0
MBK_RENDER_SMOOTH = 1
MBK_RENDER_DISTANCE = 3
MBK_RENDER_DISTANCE_REL = 4
MBK_RENDER_EQUALIZED = 5
RENDER_SOURCES = {"bytes": MBK_RENDER_BYTES, "smooth": MBK_RENDER_SMOOTH, "distance": MBK_RENDER_DISTANCE,
                  "distance_rel": MBK_RENDER_DISTANCE_REL, "equalized": MBK_RENDER_EQUALIZED}
MBK_HISTOGRAM_MAX_MRD = 1 << 20
RENDER_SUPERSAMPLES = (1, 2, 3, 4, 8)
MBK_RENDER_BAND_BYTES = 256 << 20
# reason codes of an invalid chunk stream (include/mbk.h, "Stored chunks")
MBK_STREAM_OK, MBK_STREAM_BAD_CODEC, MBK_STREAM_BAD_SIZE, MBK_STREAM_ZERO_RUN, MBK_STREAM_TOO_LONG, MBK_STREAM_TOO_SHORT = range(6)
STREAM_REASONS = {MBK_STREAM_OK: "MBK_STREAM_OK", MBK_STREAM_BAD_CODEC: "MBK_STREAM_BAD_CODEC", MBK_STREAM_BAD_SIZE: "MBK_STREAM_BAD_SIZE",
                  MBK_STREAM_ZERO_RUN: "MBK_STREAM_ZERO_RUN", MBK_STREAM_TOO_LONG: "MBK_STREAM_TOO_LONG",
                  MBK_STREAM_TOO_SHORT: "MBK_STREAM_TOO_SHORT"}
CHUNK_SCALES = (1, 2, 4, 8, 16, 32, 64)
# density views (include/mbk.h, "Density views")
MBK_DENSITY_MAX_CELLS = 1 << 28
MBK_DENSITY_LINEAR = 0
MBK_DENSITY_SQRT = 1
DENSITY_MODES = {"linear": MBK_DENSITY_LINEAR, "sqrt": MBK_DENSITY_SQRT}
DENSITY_FACTORS = (1, 2, 4, 8)


class mbk_view(C.Structure):
    _fields_ = [("start_r", C.c_double), ("start_i", C.c_double),
                ("range_r", C.c_double), ("range_i", C.c_double),
                ("width", C.c_uint32), ("height", C.c_uint32),
                ("col0", C.c_uint32), ("row0", C.c_uint32),
                ("ncols", C.c_uint32), ("nrows", C.c_uint32)]


class mbk_deep_view(C.Structure):
    _fields_ = [("range_r", C.c_double), ("range_i", C.c_double),
                ("width", C.c_uint32), ("height", C.c_uint32),
                ("col0", C.c_uint32), ("row0", C.c_uint32),
                ("ncols", C.c_uint32), ("nrows", C.c_uint32)]


class mbk_deep_xview(C.Structure):
    _fields_ = [("range_r", C.c_double), ("range_i", C.c_double), ("exp2", C.c_int32),
                ("width", C.c_uint32), ("height", C.c_uint32),
                ("col0", C.c_uint32), ("row0", C.c_uint32),
                ("ncols", C.c_uint32), ("nrows", C.c_uint32)]


class mbk_render_spec(C.Structure):
    _fields_ = [("source", C.c_uint32), ("supersample", C.c_uint32), ("palette", C.c_void_p),
                ("palette_len", C.c_uint32), ("inside", C.c_uint8 * 4),
                ("scale", C.c_double), ("offset", C.c_double), ("max_band_rows", C.c_uint32)]


class mbk_chunk_spec(C.Structure):
    _fields_ = [("palette", C.c_void_p), ("scale", C.c_uint32)]


class mbk_interior_render_spec(C.Structure):
    _fields_ = [("supersample", C.c_uint32), ("palette", C.c_void_p), ("palette_len", C.c_uint32),
                ("unknown", C.c_uint8 * 4), ("outside", C.c_uint8 * 4), ("scale", C.c_double), ("max_band_rows", C.c_uint32)]


class mbk_relief_spec(C.Structure):
    _fields_ = [("supersample", C.c_uint32), ("palette", C.c_void_p), ("palette_len", C.c_uint32), ("inside", C.c_uint8 * 4),
                ("scale", C.c_double), ("offset", C.c_double), ("light_x", C.c_double), ("light_y", C.c_double),
                ("height", C.c_double), ("max_band_rows", C.c_uint32)]


class mbk_stripe_state(C.Structure):
    _fields_ = [("S", C.c_double), ("t_last", C.c_double), ("mag", C.c_double), ("v", C.c_double), ("n", C.c_int32),
                ("N", C.c_int32), ("cnt", C.c_int32), ("reserved", C.c_int32)]


class mbk_stripe_spec(C.Structure):
    _fields_ = [("supersample", C.c_uint32), ("palette", C.c_void_p), ("palette_len", C.c_uint32), ("inside", C.c_uint8 * 4),
                ("scale", C.c_double), ("offset", C.c_double), ("density", C.c_uint32), ("skip", C.c_uint32),
                ("lo", C.c_double), ("gain", C.c_double), ("max_band_rows", C.c_uint32)]


class mbk_density_target(C.Structure):
    _fields_ = [("start_r", C.c_double), ("start_i", C.c_double), ("range_r", C.c_double), ("range_i", C.c_double),
                ("width", C.c_uint32), ("height", C.c_uint32)]


class mbk_density_stats(C.Structure):
    _fields_ = [("deposits", C.c_uint64), ("dropped", C.c_uint64)]


class mbk_density_render_spec(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("factor", C.c_uint32), ("palette", C.c_void_p), ("palette_len", C.c_uint32),
                ("scale", C.c_double), ("offset", C.c_double)]


class mbk_stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_float), ("d2h_ms", C.c_float),
                ("pixel_iterations", C.c_uint64), ("never_pixels", C.c_uint64),
                ("all_bytes_zero", C.c_uint32), ("all_bytes_one", C.c_uint32),
                ("rle_runs", C.c_uint64)]


class mbk_device_info(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("arch", C.c_char * 64),
                ("compute_units", C.c_int), ("clock_mhz", C.c_int),
                ("wavefront_size", C.c_int), ("total_mem", C.c_uint64)]


class mbk_worker_report(C.Structure):
    _fields_ = [("leased", C.c_uint64), ("accepted", C.c_uint64), ("rejected", C.c_uint64), ("resets", C.c_uint64),
                ("uniform_tiles", C.c_uint64), ("pixel_iterations", C.c_uint64),
                ("kernel_ms_sum", C.c_double), ("seconds", C.c_double), ("net_retries", C.c_uint64)]


# enum mbk_net_option (include/mbk.h), in order: process-wide network behaviour of the native worker loop
NET_OPTIONS = {name: i for i, name in enumerate(
    ["max_connections", "connect_timeout_ms", "io_timeout_ms", "retries", "backoff_ms", "stop", "peak_connections", "feeder_slots"])}


FEEDER_SUBMIT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)
FEEDER_WAIT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(mbk_stats))
FEEDER_ALLOC = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_uint64)
FEEDER_RELEASE = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
FEEDER_ON_TILE = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint32 * 4), C.POINTER(mbk_stats), C.c_int)


class mbk_feeder_ops(C.Structure):
    _fields_ = [("user", C.c_void_p), ("submit", FEEDER_SUBMIT), ("wait", FEEDER_WAIT), ("alloc", FEEDER_ALLOC),
                ("release", FEEDER_RELEASE), ("on_tile", FEEDER_ON_TILE)]


# symbol -> (restype, argtypes); this table is also what tests/test_abi.py checks against mbk.h
SIGNATURES = {
    "mbk_abi_version": (C.c_int, []),
    "mbk_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "mbk_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "mbk_destroy": (None, [C.c_void_p]),
    "mbk_last_error": (C.c_char_p, [C.c_void_p]),
    "mbk_get_device_info": (C.c_int, [C.c_void_p, C.POINTER(mbk_device_info)]),
    "mbk_device_pci_bus_id": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "mbk_host_alloc": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "mbk_host_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mbk_datachunk_geometry": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(C.c_double)]),
    "mbk_view_outside_circle": (C.c_int, [C.POINTER(mbk_view), C.c_uint32, C.POINTER(C.c_int)]),
    "mbk_view_needs_literal_doubling": (C.c_int, [C.POINTER(mbk_view), C.c_uint32, C.POINTER(C.c_int)]),
    "mbk_view_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_view_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_datachunk": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_view_launch_smooth": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_view_compute_smooth": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_view_launch_distance": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_view_compute_distance": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_distance_value_host": (C.c_double, [C.c_double, C.c_double, C.c_int32]),
    "mbk_datachunk_submit": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_void_p]),
    "mbk_datachunk_submit_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_uint32]),
    "mbk_view_submit": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                  C.c_void_p, C.c_void_p]),
    "mbk_wait": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(mbk_stats)]),
    "mbk_serialize_last": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint32)]),
    "mbk_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32]),
    "mbk_get_option": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]),
    "mbk_quantise_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    "mbk_units_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mbk_units_lookup": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mbk_sure_interior_point": (C.c_int, [C.c_double, C.c_double]),
    "mbk_sure_interior_blocks": (C.c_int, [C.POINTER(mbk_view), C.POINTER(C.c_uint64)]),
    "mbk_sure_interior_flag": (C.c_int, [C.POINTER(mbk_view), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_uint32)]),
    "mbk_reduce_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                    C.POINTER(mbk_stats)]),
    "mbk_worker_run": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint16, C.c_uint64, C.c_uint32,
                                 C.POINTER(mbk_worker_report)]),
    "mbk_net_set_option": (C.c_int, [C.c_int, C.c_uint32]),
    "mbk_net_get_option": (C.c_int, [C.c_int, C.POINTER(C.c_uint32)]),
    "mbk_feeder_run": (C.c_int, [C.POINTER(mbk_feeder_ops), C.c_char_p, C.c_uint16, C.c_uint64, C.c_uint32,
                                 C.POINTER(mbk_worker_report)]),
    "mbk_deep_orbit_create": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mbk_deep_orbit_destroy": (None, [C.c_void_p]),
    "mbk_deep_orbit_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32)]),
    "mbk_deep_orbit_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "mbk_deep_view_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_deep_view_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_view_submit": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_void_p]),
    "mbk_deep_view_launch_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_deep_view_compute_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                 C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_distance_value_host": (C.c_double, [C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32]),
    "mbk_deep_view_launch_nucleus": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_deep_view_compute_nucleus": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_nucleus_host": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_double)]),
    "mbk_deep_orbit_newton_host": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                             C.POINTER(C.c_int32)]),
    "mbk_deep_orbit_size_host": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_int32)]),
    "mbk_deep_view_launch_distance_bla": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_deep_view_compute_distance_bla": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                     C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_view_distance_bla_render_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                           C.POINTER(mbk_render_spec), C.c_void_p, C.c_void_p]),
    "mbk_deep_view_distance_bla_render_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                            C.POINTER(mbk_render_spec), C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_distance_bla_host": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                             C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "mbk_deep_distance_bla_skip_host": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double),
                                                  C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "mbk_deep_bla_info": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_view), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "mbk_deep_bla_read": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_uint64]),
    "mbk_deep_bla_count_host": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "mbk_deep_orbit_read_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "mbk_deep_xview_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_deep_xview_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_xview_submit": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p]),
    "mbk_deep_xview_count_host": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "mbk_deep_xview_launch_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_deep_xview_compute_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                  C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_xview_distance_host": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                               C.POINTER(C.c_double)]),
    "mbk_deep_xdistance_step_host": (C.c_int, [C.c_double, C.c_double, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                               C.POINTER(C.c_int32)]),
    "mbk_deep_xdistance_value_host": (C.c_double, [C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int32]),
    "mbk_deep_xview_launch_nucleus": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_deep_xview_compute_nucleus": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_xview_nucleus_host": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                              C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                              C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "mbk_deep_xview_distance_render_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                        C.POINTER(mbk_render_spec), C.c_void_p, C.c_void_p]),
    "mbk_deep_xview_distance_render_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                         C.POINTER(mbk_render_spec), C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_xview_launch_distance_xbla": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_deep_xview_compute_distance_xbla": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                       C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_xview_distance_xbla_render_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32,
                                                             C.c_uint32, C.POINTER(mbk_render_spec), C.c_void_p, C.c_void_p]),
    "mbk_deep_xview_distance_xbla_render_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32,
                                                              C.c_uint32, C.POINTER(mbk_render_spec), C.c_void_p,
                                                              C.POINTER(mbk_stats)]),
    "mbk_deep_xview_distance_xbla_host": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                                    C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                                    C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "mbk_deep_xdistance_skip_host": (C.c_int, [C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                               C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "mbk_deep_xbla_info": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_xview), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "mbk_deep_xbla_read": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "mbk_deep_xbla_count_host": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "mbk_deep_xview_render_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                               C.POINTER(mbk_render_spec), C.c_void_p, C.c_void_p]),
    "mbk_deep_xview_render_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                C.POINTER(mbk_render_spec), C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_xview_render_equalized_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                         C.POINTER(mbk_render_spec), C.c_void_p, C.c_uint32, C.c_void_p,
                                                         C.c_void_p]),
    "mbk_deep_xview_render_equalized_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32,
                                                          C.c_uint32, C.POINTER(mbk_render_spec), C.c_void_p, C.c_uint32,
                                                          C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_xview_histogram_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                  C.c_void_p, C.c_void_p]),
    "mbk_deep_xview_histogram_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                   C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_view_render_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                         C.POINTER(mbk_render_spec), C.c_void_p, C.c_void_p]),
    "mbk_view_render_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                          C.POINTER(mbk_render_spec), C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_view_render_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                              C.POINTER(mbk_render_spec), C.c_void_p, C.c_void_p]),
    "mbk_deep_view_render_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                               C.POINTER(mbk_render_spec), C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_palette_viewer": (C.c_int, [C.c_void_p]),
    "mbk_render_resolve_host": (C.c_int, [C.POINTER(mbk_render_spec), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "mbk_view_render_adaptive_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                                  C.POINTER(mbk_render_spec), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_view_render_adaptive_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                                   C.POINTER(mbk_render_spec), C.c_uint32, C.c_void_p, C.c_void_p,
                                                   C.POINTER(mbk_stats)]),
    "mbk_render_adaptive_host": (C.c_int, [C.POINTER(mbk_render_spec), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_deep_view_render_adaptive_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                       C.POINTER(mbk_render_spec), C.c_uint32, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]),
    "mbk_deep_view_render_adaptive_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                        C.POINTER(mbk_render_spec), C.c_uint32, C.c_void_p, C.c_void_p,
                                                        C.POINTER(mbk_stats)]),
    "mbk_deep_xview_render_adaptive_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                        C.POINTER(mbk_render_spec), C.c_uint32, C.c_void_p, C.c_void_p,
                                                        C.c_void_p]),
    "mbk_deep_xview_render_adaptive_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                         C.POINTER(mbk_render_spec), C.c_uint32, C.c_void_p, C.c_void_p,
                                                         C.POINTER(mbk_stats)]),
    "mbk_counts_histogram": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mbk_view_histogram_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mbk_deep_view_histogram_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                 C.c_void_p, C.c_void_p]),
    "mbk_view_histogram_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32, C.c_void_p,
                                             C.POINTER(mbk_stats)]),
    "mbk_deep_view_histogram_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                  C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_counts_histogram_host": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    "mbk_equalize_lut_host": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "mbk_equalize_value_host": (C.c_double, [C.c_void_p, C.c_uint32, C.c_double]),
    "mbk_view_render_equalized_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                                   C.POINTER(mbk_render_spec), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mbk_view_render_equalized_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                                    C.POINTER(mbk_render_spec), C.c_void_p, C.c_uint32, C.c_void_p,
                                                    C.POINTER(mbk_stats)]),
    "mbk_deep_view_render_equalized_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                        C.POINTER(mbk_render_spec), C.c_void_p, C.c_uint32, C.c_void_p,
                                                        C.c_void_p]),
    "mbk_deep_view_render_equalized_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                         C.POINTER(mbk_render_spec), C.c_void_p, C.c_uint32, C.c_void_p,
                                                         C.POINTER(mbk_stats)]),
    "mbk_render_resolve_equalized_host": (C.c_int, [C.POINTER(mbk_render_spec), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_julia_view_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_julia_view_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_julia_view_submit": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p]),
    "mbk_julia_view_render_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                               C.POINTER(mbk_render_spec), C.c_void_p, C.c_void_p]),
    "mbk_julia_view_render_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                                C.POINTER(mbk_render_spec), C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_julia_view_render_equalized_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32,
                                                         C.c_uint32, C.POINTER(mbk_render_spec), C.c_void_p, C.c_uint32,
                                                         C.c_void_p, C.c_void_p]),
    "mbk_julia_view_render_equalized_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32,
                                                          C.c_uint32, C.POINTER(mbk_render_spec), C.c_void_p, C.c_uint32,
                                                          C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_julia_view_histogram_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                                  C.c_void_p, C.c_void_p]),
    "mbk_julia_view_histogram_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                                   C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_julia_count_host": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint32, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_double)]),
    "mbk_julia_view_launch_distance": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_julia_view_compute_distance": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                                  C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_julia_view_distance_render_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32,
                                                        C.c_uint32, C.POINTER(mbk_render_spec), C.c_void_p, C.c_void_p]),
    "mbk_julia_view_distance_render_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_double, C.c_double, C.c_uint32,
                                                         C.c_uint32, C.POINTER(mbk_render_spec), C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_julia_distance_host": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint32, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32)] + [C.POINTER(C.c_double)] * 7),
    "mbk_view_interior_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "mbk_view_interior_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_interior_host": (C.c_int, [C.c_double, C.c_double, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "mbk_view_interior_render_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                                  C.POINTER(mbk_interior_render_spec), C.c_void_p, C.c_void_p]),
    "mbk_view_interior_render_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                                   C.POINTER(mbk_interior_render_spec), C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_interior_resolve_host": (C.c_int, [C.POINTER(mbk_interior_render_spec), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "mbk_view_launch_normal": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "mbk_view_compute_normal": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_normal_value_host": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, C.POINTER(C.c_double)]),
    "mbk_relief_shade_host": (C.c_uint32, [C.c_double] * 5),
    "mbk_view_relief_render_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                                C.POINTER(mbk_relief_spec), C.c_void_p, C.c_void_p]),
    "mbk_view_relief_render_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                                 C.POINTER(mbk_relief_spec), C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_relief_resolve_host": (C.c_int, [C.POINTER(mbk_relief_spec), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "mbk_view_launch_stripe": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_view_compute_stripe": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_stripe_state_host": (C.c_int, [C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(mbk_stripe_state)]),
    "mbk_stripe_value_host": (C.c_double, [C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32]),
    "mbk_stripe_shade_host": (C.c_uint32, [C.c_double] * 3),
    "mbk_view_stripe_render_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                                C.POINTER(mbk_stripe_spec), C.c_void_p, C.c_void_p]),
    "mbk_view_stripe_render_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.c_uint32, C.c_uint32,
                                                 C.POINTER(mbk_stripe_spec), C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_stripe_resolve_host": (C.c_int, [C.POINTER(mbk_stripe_spec), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "mbk_deep_view_launch_normal": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_deep_view_compute_normal": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_view_relief_render_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                     C.POINTER(mbk_relief_spec), C.c_void_p, C.c_void_p]),
    "mbk_deep_view_relief_render_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32,
                                                      C.POINTER(mbk_relief_spec), C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_normal_host": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_view), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "mbk_deep_xview_launch_normal": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_deep_xview_compute_normal": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_xview_relief_render_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                      C.POINTER(mbk_relief_spec), C.c_void_p, C.c_void_p]),
    "mbk_deep_xview_relief_render_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32,
                                                       C.POINTER(mbk_relief_spec), C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_deep_xview_normal_host": (C.c_int, [C.c_void_p, C.POINTER(mbk_deep_xview), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                             C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "mbk_view_density_launch": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.POINTER(mbk_density_target), C.c_uint32, C.c_uint32,
                                          C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mbk_view_density_compute": (C.c_int, [C.c_void_p, C.POINTER(mbk_view), C.POINTER(mbk_density_target), C.c_uint32, C.c_uint32,
                                           C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(mbk_stats),
                                           C.POINTER(mbk_density_stats)]),
    "mbk_density_max": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p]),
    "mbk_density_render_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(mbk_density_render_spec),
                                            C.c_void_p, C.c_void_p]),
    "mbk_density_render_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(mbk_density_render_spec),
                                             C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_density_cell_host": (C.c_int, [C.POINTER(mbk_density_target), C.c_double, C.c_double, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "mbk_density_accumulate_host": (C.c_int, [C.POINTER(mbk_view), C.POINTER(mbk_density_target), C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.POINTER(mbk_density_stats)]),
    "mbk_density_resolve_host": (C.c_int, [C.POINTER(mbk_density_render_spec), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mbk_density_build_info": (C.c_int, []),
    "mbk_chunk_stream_check": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32)]),
    "mbk_chunk_decode_host": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "mbk_chunk_resolve_host": (C.c_int, [C.POINTER(mbk_chunk_spec), C.c_void_p, C.c_void_p, C.c_uint64]),
    "mbk_chunk_decode_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mbk_chunk_render_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(mbk_chunk_spec), C.c_void_p, C.c_uint64,
                                          C.c_void_p, C.c_void_p]),
    "mbk_chunk_decode_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(mbk_stats)]),
    "mbk_chunk_render_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(mbk_chunk_spec), C.c_void_p, C.c_uint64,
                                           C.POINTER(mbk_stats)]),
}

_lib = None


def _share_hip_runtime_with_torch() -> None:
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.7 (same SONAME as /opt/rocm's).  Whichever
    copy is loaded first serves the whole process; torch fails with "No HIP GPUs are available" when
    the system copy got in first.  So: if torch is installed but not imported yet, pre-load ITS copy
    (cheap -- torch itself is not imported) so that either import order works.  Opt out with
    MBK_HIP_RUNTIME=system."""
    if os.environ.get("MBK_HIP_RUNTIME", "") == "system" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load() -> C.CDLL:
    """Load libmbk_hip.so and declare every entry point.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError(
            f"{SO_PATH} is missing: build it with `python -m distributedmandelbrot_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(SO_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.mbk_abi_version() != MBK_ABI_VERSION:
        raise ImportError("libmbk_hip.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib
