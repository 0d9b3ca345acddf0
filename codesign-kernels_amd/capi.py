"""ctypes binding of libmpdata_hip.so (include/mpdata_hip.h) and the Python
mirror of the reference's operator interface.

Array convention.  The reference declares (Fortran, column-major, `sl`
fastest; reference :479-484, :30)
    f(ncrms,-2:nx+3,1,nzm)  u(ncrms,-1:nx+3,1,nzm)  w(ncrms,-1:nx+2,1,nz)
    rho(ncrms,nzm)  rhow(ncrms,nz)  adz(ncrms,nzm)  flux(ncrms,nz)
The same bytes are
  * numpy: Fortran-ordered arrays of shape (ncrms, nx+6, nzm[, ntracers]) ...
  * torch: C-contiguous tensors with the axes reversed,
           ([ntracers,] nzm, nx+6, ncrms) ...
so a device tensor's last axis is the coalesced CRM-instance axis.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MPDATA_HIP_LIB: load an alternative build of the library (kernel experiments)
_LIB_PATH = os.environ.get("MPDATA_HIP_LIB") or os.path.join(HERE, "libmpdata_hip.so")
VARIANT_EXACT, VARIANT_FAST = 0, 1
EINVAL, EUNSUPPORTED, ESTATE, ECOMM = -1, -2, -3, -4   # MPDATA_E* of include/mpdata_hip.h
LAYOUT_REFERENCE, LAYOUT_WAVEMAJOR = 0, 1
BOUNDARY_GIVEN, BOUNDARY_PERIODIC = 0, 1   # MPDATA_BOUNDARY_* (include/mpdata_hip.h section 3a)
LEVEL_ADD, LEVEL_ADD_CLIP = 0, 1           # MPDATA_LEVEL_ADD* (include/mpdata_hip.h section 3i)
CELL_ADD, CELL_ADD_CLIP = 0, 1             # MPDATA_CELL_ADD* (include/mpdata_hip.h section 3p)
CONVERT_LIMIT = 1                          # MPDATA_CONVERT_LIMIT (include/mpdata_hip.h section 3t)
COMBINE_CLIP, COMBINE_MAX = 1, 8            # MPDATA_COMBINE_* (include/mpdata_hip.h section 3z)
LEVEL_HIST_MAX_BINS = 32   # MPDATA_LEVEL_HIST_MAX_BINS (include/mpdata_hip.h section 3ab)
COLUMN_SCAN_DOWN, COLUMN_SCAN_EXCLUSIVE = 1, 2   # MPDATA_COLUMN_SCAN_* (include/mpdata_hip.h section 3aa)
SATADJ_ICE = 1                             # MPDATA_SATADJ_ICE (include/mpdata_hip.h section 3y)
LEVEL_COV_RAW = 1                          # MPDATA_LEVEL_COV_RAW (include/mpdata_hip.h section 3u)

_lib = None


class MpdataError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmpdata_hip error {code}: {msg}")
        self.code = code


class SatadjParams(ctypes.Structure):
    """struct mpdata_satadj_params (include/mpdata_hip.h section 3y): the caller's numbers of a saturation adjustment.
    SatadjParams(esw=[...9], desw=[...9], esi=[...9], desi=[...9], t0=..., xmin=..., eps=..., lv=..., ls=..., tmin=...,
    tmax=..., tol=..., maxit=...); what is not given is 0."""
    _fields_ = [("esw", ctypes.c_double * 9), ("desw", ctypes.c_double * 9), ("esi", ctypes.c_double * 9),
                ("desi", ctypes.c_double * 9), ("t0", ctypes.c_double), ("xmin", ctypes.c_double), ("eps", ctypes.c_double),
                ("lv", ctypes.c_double), ("ls", ctypes.c_double), ("tmin", ctypes.c_double), ("tmax", ctypes.c_double),
                ("tol", ctypes.c_double), ("maxit", ctypes.c_int)]

    def __init__(self, **kw):
        super().__init__()
        for k, v in kw.items():
            if k in ("esw", "desw", "esi", "desi"):
                v = [float(x) for x in v]
                if len(v) != 9:
                    raise MpdataError(-1, f"SatadjParams: {k} has {len(v)} coefficients, not 9")
                v = (ctypes.c_double * 9)(*v)
            elif k not in dict(self._fields_):
                raise MpdataError(-1, f"SatadjParams: no field {k}")
            setattr(self, k, v)


def lib_path():
    return _LIB_PATH


def build_library(force=False):
    """hipcc --offload-arch=gfx950 the kernels + C-ABI into libmpdata_hip.so
    (cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(HERE, "csrc"), "-j4"]
    if force:
        args.append("-B")
    subprocess.run(args, check=True, stdout=subprocess.DEVNULL)
    return _LIB_PATH


def lib():
    """The loaded library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise MpdataError(-100, f"{_LIB_PATH} not built; run __graft_entry__.build() "
                                    "(make -C codesign-kernels_amd/csrc)")
        L = ctypes.CDLL(_LIB_PATH)
        dp, vp = ctypes.c_void_p, ctypes.c_void_p
        i64, ci = ctypes.c_int64, ctypes.c_int
        L.mpdata_advect_scalar2d.restype = ci
        L.mpdata_advect_scalar2d.argtypes = [i64, ci, ci, ci] + [dp] * 7
        L.mpdata_advect_scalar2d_device.restype = ci
        L.mpdata_advect_scalar2d_device.argtypes = [i64, ci, ci, ci] + [dp] * 7 + [vp]
        L.mpdata_plan_create.restype = ci
        L.mpdata_plan_create.argtypes = [i64, ci, ci, ci, ctypes.POINTER(vp)]
        L.mpdata_plan_upload.restype = ci
        L.mpdata_plan_upload.argtypes = [vp] + [dp] * 7
        for name in ("mpdata_plan_run", "mpdata_plan_sync", "mpdata_plan_destroy"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp]
        L.mpdata_plan_download.restype = ci
        L.mpdata_plan_download.argtypes = [vp, dp, dp]
        L.mpdata_plan_last_kernel_ms.restype = ci
        L.mpdata_plan_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.mpdata_plan_run_tracers.restype = ci
        L.mpdata_plan_run_tracers.argtypes = [vp, ci, ci]
        L.mpdata_plan_set_timing.restype = ci
        L.mpdata_plan_set_timing.argtypes = [vp, ci]
        L.mpdata_plan_run_uw.restype = ci
        L.mpdata_plan_run_uw.argtypes = [vp, ci, ci, vp, vp]
        L.mpdata_plan_import_device.restype = ci
        L.mpdata_plan_import_device.argtypes = [vp] + [vp] * 7 + [ci, ci]
        L.mpdata_plan_export_device.restype = ci
        L.mpdata_plan_export_device.argtypes = [vp, vp, vp, ci, ci]
        L.mpdata_plan_import_instances_device.restype = ci
        L.mpdata_plan_import_instances_device.argtypes = [vp, i64, i64] + [vp] * 7 + [ci, ci]
        L.mpdata_plan_export_instances_device.restype = ci
        L.mpdata_plan_export_instances_device.argtypes = [vp, i64, i64, vp, vp, ci, ci]
        for name in ("mpdata_plan_download_instances", "mpdata_plan_download_instances_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, dp]
        L.mpdata_plan_level_stats_device.restype = ci
        L.mpdata_plan_level_stats_device.argtypes = [vp, i64, i64, vp, vp, vp, ci, ci]
        for name in ("mpdata_plan_level_stats", "mpdata_plan_level_stats_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, dp, dp]
        for name in ("mpdata_level_stats_device", "mpdata_level_stats_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, dp, dp, dp, dp, vp]
        L.mpdata_plan_courant_device.restype = ci
        L.mpdata_plan_courant_device.argtypes = [vp, i64, i64, vp, vp]
        for name in ("mpdata_plan_courant", "mpdata_plan_courant_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, dp]
        for name in ("mpdata_courant_device", "mpdata_courant_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, dp, dp, dp, dp, dp, dp, vp]
        L.mpdata_plan_level_add_device.restype = ci
        L.mpdata_plan_level_add_device.argtypes = [vp, i64, i64, vp, ci, ci, ci]
        for name in ("mpdata_plan_level_add", "mpdata_plan_level_add_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, ci]
        for name in ("mpdata_level_add_device", "mpdata_level_add_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, dp, dp, ci, vp]
        L.mpdata_plan_scale_uw_device.restype = ci
        L.mpdata_plan_scale_uw_device.argtypes = [vp, i64, i64, vp, vp]
        for name in ("mpdata_plan_scale_uw", "mpdata_plan_scale_uw_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, dp]
        for name in ("mpdata_scale_uw_device", "mpdata_scale_uw_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, dp, dp, dp, dp, vp]
        L.mpdata_plan_column_path_device.restype = ci
        L.mpdata_plan_column_path_device.argtypes = [vp, i64, i64, vp, vp, ci, ci]
        for name in ("mpdata_plan_column_path", "mpdata_plan_column_path_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, dp]
        for name in ("mpdata_column_path_device", "mpdata_column_path_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, dp, dp, dp, dp, dp, vp]
        L.mpdata_plan_diffuse_device.restype = ci
        L.mpdata_plan_diffuse_device.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, vp, ci, ci]
        for name in ("mpdata_plan_diffuse", "mpdata_plan_diffuse_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, dp, dp, dp, dp, dp]
        for name in ("mpdata_diffuse_device", "mpdata_diffuse_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64] + [dp] * 9 + [vp]
        L.mpdata_plan_subside_device.restype = ci
        L.mpdata_plan_subside_device.argtypes = [vp, i64, i64, vp, vp, vp, ci, ci]
        for name in ("mpdata_plan_subside", "mpdata_plan_subside_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, dp, dp]
        for name in ("mpdata_subside_device", "mpdata_subside_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, dp, dp, dp, dp, vp]
        L.mpdata_plan_sediment_device.restype = ci
        L.mpdata_plan_sediment_device.argtypes = [vp, i64, i64, vp, vp, vp, ci, ci]
        for name in ("mpdata_plan_sediment", "mpdata_plan_sediment_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, dp, dp]
        for name in ("mpdata_sediment_device", "mpdata_sediment_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64] + [dp] * 6 + [vp]
        L.mpdata_plan_vsolve_device.restype = ci
        L.mpdata_plan_vsolve_device.argtypes = [vp, i64, i64, vp, vp, vp, ci, ci]
        for name in ("mpdata_plan_vsolve", "mpdata_plan_vsolve_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, dp, dp]
        for name in ("mpdata_vsolve_device", "mpdata_vsolve_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64] + [dp] * 4 + [vp]
        L.mpdata_plan_cell_add_device.restype = ci
        L.mpdata_plan_cell_add_device.argtypes = [vp, i64, i64, vp, ctypes.c_double, ci, vp, ci, ci]
        for name, cf in (("mpdata_plan_cell_add", ctypes.c_double), ("mpdata_plan_cell_add_f32", ctypes.c_float)):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, cf, ci, dp]
        for name, cf in (("mpdata_cell_add_device", ctypes.c_double), ("mpdata_cell_add_f32_device", ctypes.c_float)):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64, dp, dp, cf, ci, dp, vp]
        L.mpdata_plan_column_step_device.restype = ci
        L.mpdata_plan_column_step_device.argtypes = [vp, i64, i64, vp, ctypes.c_double, ci] + [vp] * 7 + [ci, ci]
        for name, cf in (("mpdata_plan_column_step", ctypes.c_double), ("mpdata_plan_column_step_f32", ctypes.c_float)):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, cf, ci] + [dp] * 7
        for name, cf in (("mpdata_column_step_device", ctypes.c_double), ("mpdata_column_step_f32_device", ctypes.c_float)):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64, dp, dp, dp, dp, cf, ci] + [dp] * 7 + [vp]
        L.mpdata_plan_relax_device.restype = ci
        L.mpdata_plan_relax_device.argtypes = [vp, i64, i64, vp, vp, vp, ci, ci]
        for name in ("mpdata_plan_relax", "mpdata_plan_relax_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, dp, dp]
        for name in ("mpdata_relax_device", "mpdata_relax_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64] + [dp] * 4 + [vp]
        L.mpdata_plan_vdiffuse_device.restype = ci
        L.mpdata_plan_vdiffuse_device.argtypes = [vp, i64, i64, vp, vp, vp, vp, ci, ci]
        for name in ("mpdata_plan_vdiffuse", "mpdata_plan_vdiffuse_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, dp, dp, dp]
        for name in ("mpdata_vdiffuse_device", "mpdata_vdiffuse_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64] + [dp] * 7 + [vp]
        L.mpdata_plan_convert_device.restype = ci
        L.mpdata_plan_convert_device.argtypes = [vp, i64, i64, ci, ci, vp, vp, vp, ci, vp]
        for name in ("mpdata_plan_convert", "mpdata_plan_convert_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, ci, ci, dp, dp, dp, ci, dp]
        for name in ("mpdata_convert_device", "mpdata_convert_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64, dp, ci, ci, dp, dp, dp, ci, dp, vp]
        L.mpdata_plan_level_cov_device.restype = ci
        L.mpdata_plan_level_cov_device.argtypes = [vp, i64, i64, ci, ci, vp, vp, ci, vp, vp, vp]
        for name in ("mpdata_plan_level_cov", "mpdata_plan_level_cov_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, ci, ci, dp, dp, ci, dp, dp, dp]
        for name in ("mpdata_level_cov_device", "mpdata_level_cov_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64, dp, ci, ci, dp, dp, ci, dp, dp, dp, vp]
        L.mpdata_plan_level_cond_device.restype = ci
        L.mpdata_plan_level_cond_device.argtypes = [vp, i64, i64, ci, vp, vp, vp, vp, ci, ci]
        for name in ("mpdata_plan_level_cond", "mpdata_plan_level_cond_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, ci, dp, dp, dp, dp]
        for name in ("mpdata_level_cond_device", "mpdata_level_cond_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64, dp, ci, dp, dp, dp, dp, ci, ci, vp]
        L.mpdata_plan_column_cond_device.restype = ci
        L.mpdata_plan_column_cond_device.argtypes = [vp, i64, i64, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci]
        for name in ("mpdata_plan_column_cond", "mpdata_plan_column_cond_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, ci, dp, dp, dp, dp, dp, dp, dp, dp]
        for name in ("mpdata_column_cond_device", "mpdata_column_cond_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64, dp, dp, dp, ci, dp, dp, dp, dp, dp, dp, dp, dp, ci, ci, vp]
        L.mpdata_plan_nonneg_device.restype = ci
        L.mpdata_plan_nonneg_device.argtypes = [vp, i64, i64, vp, vp, ci, ci]
        for name in ("mpdata_plan_nonneg", "mpdata_plan_nonneg_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, dp, dp]
        for name in ("mpdata_nonneg_device", "mpdata_nonneg_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64, dp, dp, dp, vp]
        pp = ctypes.POINTER(SatadjParams)
        L.mpdata_plan_satadj_device.restype = ci
        L.mpdata_plan_satadj_device.argtypes = [vp, i64, i64, ci, ci, ci, ci, vp, vp, pp, ci, vp, vp]
        for name in ("mpdata_plan_satadj", "mpdata_plan_satadj_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, ci, ci, ci, ci, dp, dp, pp, ci, dp, dp]
        for name in ("mpdata_satadj_device", "mpdata_satadj_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64, dp, ci, ci, ci, ci, dp, dp, pp, ci, dp, dp, vp]
        ip = ctypes.c_void_p                    # const int* src: a host array (_src_arg)
        L.mpdata_plan_combine_device.restype = ci
        L.mpdata_plan_combine_device.argtypes = [vp, i64, i64, ci, ci, ip, vp, vp, ci, vp]
        for name in ("mpdata_plan_combine", "mpdata_plan_combine_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, ci, ci, ip, dp, dp, ci, dp]
        for name in ("mpdata_combine_device", "mpdata_combine_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64, dp, ci, ci, ip, dp, dp, ci, dp, vp]
        L.mpdata_plan_column_scan_device.restype = ci
        L.mpdata_plan_column_scan_device.argtypes = [vp, i64, i64, ci, ci, vp, vp, ci]
        for name in ("mpdata_plan_column_scan", "mpdata_plan_column_scan_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, ci, ci, dp, dp, ci]
        for name in ("mpdata_column_scan_device", "mpdata_column_scan_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64, dp, ci, ci, dp, dp, ci, vp]
        ep = ctypes.c_void_p                    # const double* edges: a host array (_edges_arg)
        L.mpdata_plan_level_hist_device.restype = ci
        L.mpdata_plan_level_hist_device.argtypes = [vp, i64, i64, ci, ci, ep, vp, vp, ci, ci]
        for name in ("mpdata_plan_level_hist", "mpdata_plan_level_hist_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, ci, ci, ep, dp, dp]
        for name in ("mpdata_level_hist_device", "mpdata_level_hist_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64, dp, ci, ci, ep, dp, dp, ci, ci, vp]
        cd = ctypes.c_double
        L.mpdata_plan_level_draft_device.restype = ci
        L.mpdata_plan_level_draft_device.argtypes = [vp, i64, i64, ci, vp, vp, cd, cd, vp, vp, vp, vp, ci, ci]
        for name in ("mpdata_plan_level_draft", "mpdata_plan_level_draft_f32"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp, i64, i64, ci, dp, dp, cd, cd, dp, dp, dp, dp]
        for name in ("mpdata_level_draft_device", "mpdata_level_draft_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, i64, i64, dp, dp, ci, dp, dp, cd, cd, dp, dp, dp, dp, ci, ci, vp]
        L.mpdata_plan_set_stream.restype = ci
        L.mpdata_plan_set_stream.argtypes = [vp, vp]
        for name in ("mpdata_plan_layout", "mpdata_plan_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [vp]
        L.mpdata_set_tall_columns.restype = ci
        L.mpdata_set_tall_columns.argtypes = [ci]
        L.mpdata_set_f32_odd_ncrms.restype = ci
        L.mpdata_set_f32_odd_ncrms.argtypes = [ci]
        L.mpdata_plan_level_windows.restype = ci
        L.mpdata_plan_level_windows.argtypes = [vp]
        L.mpdata_level_window.restype = ci
        L.mpdata_level_window.argtypes = [ci, ci] + [ctypes.POINTER(ci)] * 4
        L.mpdata_set_plan_layout.restype = ci
        L.mpdata_set_plan_layout.argtypes = [ci]
        L.mpdata_plan_set_boundary.restype = ci
        L.mpdata_plan_set_boundary.argtypes = [vp, ci]
        L.mpdata_plan_boundary.restype = ci
        L.mpdata_plan_boundary.argtypes = [vp]
        for name in ("mpdata_periodic_halo_device", "mpdata_periodic_halo_f32_device"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = [i64, ci, ci, ci, dp, dp, dp, vp]
        L.mpdata_plan_create_multi.restype = ci
        L.mpdata_plan_create_multi.argtypes = [i64, ci, ci, ci, ci, ctypes.POINTER(vp)]
        L.mpdata_plan_create_multi_devices.restype = ci
        L.mpdata_plan_create_multi_devices.argtypes = [i64, ci, ci, ci, ci, ctypes.POINTER(ci), ctypes.POINTER(vp)]
        L.mpdata_shard_range.restype = None
        L.mpdata_shard_range.argtypes = [i64, ci, ci, ctypes.POINTER(i64), ctypes.POINTER(i64)]
        L.mpdata_plan_ngpus.restype = ci
        L.mpdata_plan_ngpus.argtypes = [vp]
        L.mpdata_plan_ranks_seen.restype = ci
        L.mpdata_plan_ranks_seen.argtypes = [vp]
        L.mpdata_plan_shard.restype = ci
        L.mpdata_plan_shard.argtypes = [vp, ci, ctypes.POINTER(ci), ctypes.POINTER(i64), ctypes.POINTER(i64)]
        L.mpdata_plan_shard_plan.restype = vp
        L.mpdata_plan_shard_plan.argtypes = [vp, ci]
        L.mpdata_plan_transfer_stats.restype = ci
        L.mpdata_plan_transfer_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                 ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(ci)]
        L.mpdata_fill_synthetic_device.restype = ci
        L.mpdata_fill_synthetic_device.argtypes = [dp, ci, i64, i64, i64, i64, ctypes.c_uint64, ci, vp]
        L.mpdata_pack_shard_device.restype = ci
        L.mpdata_pack_shard_device.argtypes = [dp, dp, i64, i64, i64, i64, vp]
        L.mpdata_unpack_shard_device.restype = ci
        L.mpdata_unpack_shard_device.argtypes = [dp, dp, i64, i64, i64, i64, vp]
        L.mpdata_advect_scalar2d_f32.restype = ci
        L.mpdata_advect_scalar2d_f32.argtypes = [i64, ci, ci, ci] + [dp] * 7
        L.mpdata_advect_scalar2d_f32_device.restype = ci
        L.mpdata_advect_scalar2d_f32_device.argtypes = [i64, ci, ci, ci] + [dp] * 7 + [vp]
        L.mpdata_fill_synthetic_f32_device.restype = ci
        L.mpdata_fill_synthetic_f32_device.argtypes = [dp, ci, i64, i64, i64, i64, ctypes.c_uint64, ci, vp]
        L.mpdata_algorithmic_bytes_f32.restype = i64
        L.mpdata_algorithmic_bytes_f32.argtypes = [i64, ci, ci, ci]
        L.mpdata_plan_create_f32.restype = ci
        L.mpdata_plan_create_f32.argtypes = [i64, ci, ci, ci, ctypes.POINTER(vp)]
        L.mpdata_plan_upload_f32.restype = ci
        L.mpdata_plan_upload_f32.argtypes = [vp] + [dp] * 7
        L.mpdata_plan_download_f32.restype = ci
        L.mpdata_plan_download_f32.argtypes = [vp, dp, dp]
        L.mpdata_debug_stages_device.restype = ci
        L.mpdata_debug_stages_device.argtypes = [i64, ci, ci, ci] + [dp] * 11 + [vp]
        L.mpdata_set_variant.restype = ci
        L.mpdata_set_variant.argtypes = [ci]
        L.mpdata_get_variant.restype = ci
        L.mpdata_set_serpentine.restype = ci
        L.mpdata_set_serpentine.argtypes = [ci]
        L.mpdata_set_wm_flags.restype = ci
        L.mpdata_set_wm_flags.argtypes = [ci]
        L.mpdata_set_tile.restype = ci
        L.mpdata_set_tile.argtypes = [ci]
        L.mpdata_set_debug_buffer.restype = ci
        L.mpdata_set_debug_buffer.argtypes = [vp]
        L.mpdata_device_count.restype = ci
        L.mpdata_plan_device_alloc.restype = ci
        L.mpdata_plan_device_alloc.argtypes = [vp, ctypes.POINTER(vp), i64]
        L.mpdata_device_free.restype = ci
        L.mpdata_device_free.argtypes = [vp]
        L.mpdata_algorithmic_bytes.restype = i64
        L.mpdata_algorithmic_bytes.argtypes = [i64, ci, ci, ci]
        L.mpdata_diag_stream_3r1w.restype = ci
        L.mpdata_diag_stream_3r1w.argtypes = [i64, ci, ci, ctypes.POINTER(ctypes.c_double)]
        L.mpdata_last_error.restype = ctypes.c_char_p
        L.mpdata_version.restype = ctypes.c_char_p
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise MpdataError(rc, lib().mpdata_last_error().decode())


def set_variant(v):
    return lib().mpdata_set_variant(int(v))


def get_variant():
    return lib().mpdata_get_variant()


WMF_NOSTREAM, WMF_TPW1, WMF_NOSPLIT, WMF_SPLIT = 1, 2, 4, 8


def set_serpentine(on):
    """Serpentine tile order of wave-major plans (include/mpdata_hip.h section 8); returns the previous setting."""
    return lib().mpdata_set_serpentine(int(on))


def set_wm_flags(flags):
    """Test switches of the wave-major launch (WMF_*; < 0 queries); returns the previous value."""
    return lib().mpdata_set_wm_flags(int(flags))


def version():
    return lib().mpdata_version().decode()


def set_tile(t):
    return lib().mpdata_set_tile(int(t))


def set_plan_layout(layout):
    """Default device layout of new plans (LAYOUT_*); returns the previous one."""
    return lib().mpdata_set_plan_layout(int(layout))


def set_tall_columns(on):
    """Level windows for new plans (and device / host calls) with nz > 238 (include/mpdata_hip.h section 3e); returns
    the previous setting.  Off by default; MPDATA_TALL_COLUMNS=1 in the environment presets it."""
    return lib().mpdata_set_tall_columns(int(on))


def set_f32_odd_ncrms(on):
    """fp32 with an odd ncrms on the packed two-instances-per-lane kernels (include/mpdata_hip.h section 3f): new fp32
    plans at every nz the wave-major kernels cover, device / host calls from nz = 33 on; returns the previous setting.
    Off by default; MPDATA_F32_ODD_NCRMS=1 in the environment presets it."""
    return lib().mpdata_set_f32_odd_ncrms(int(on))


def level_window(nz, h):
    """(W, k0, nz_w, own0, own1): window h of the W level windows of a column of nz levels (mpdata_level_window) --
    a problem of nz_w levels on the tall levels k0+1 .. k0+nz_w-1 (+ its ghost level) that owns own0 .. own1."""
    v = [ctypes.c_int() for _ in range(4)]
    W = lib().mpdata_level_window(int(nz), int(h), *[ctypes.byref(x) for x in v])
    if W < 1:
        raise MpdataError(W, lib().mpdata_last_error().decode())
    return (W,) + tuple(x.value for x in v)


def shard_range(ncrms, ngpus, g):
    """(sl0, nloc) of GPU g's contiguous block of CRM instances (mpdata_shard_range)."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    lib().mpdata_shard_range(int(ncrms), int(ngpus), int(g), ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def stream_ceiling(bytes_per_array=538 * 2**20, nontemporal=True, iters=40):
    """GB/s of a linear 3-read-1-write stream on the current device (mpdata_diag_stream_3r1w)."""
    g = ctypes.c_double()
    _check(lib().mpdata_diag_stream_3r1w(int(bytes_per_array), int(bool(nontemporal)), int(iters), ctypes.byref(g)))
    return g.value


def device_count():
    return lib().mpdata_device_count()


def algorithmic_bytes(ncrms, nx, nz, ntracers=1, f32=False):
    fn = lib().mpdata_algorithmic_bytes_f32 if f32 else lib().mpdata_algorithmic_bytes
    return int(fn(ncrms, nx, nz, ntracers))


SID = {"adz": 0, "f": 1, "u": 2, "w": 3, "rho": 4, "rhow": 5, "flux": 6}


def shapes(ncrms, nx, nz, ntracers=1):
    """torch-side (C-order, reversed axes) shapes of the seven arrays."""
    nzm = nz - 1
    t = (ntracers,) if ntracers > 1 else ()
    return {"adz": (nzm, ncrms), "f": t + (nzm, nx + 6, ncrms), "u": (nzm, nx + 5, ncrms),
            "w": (nz, nx + 4, ncrms), "rho": (nzm, ncrms), "rhow": (nz, ncrms),
            "flux": t + (nz, ncrms)}


# Placement advice for callers that own the device arrays: a
# workgroup reads the same instance range of f, u and w at about the same time; when the
# three base addresses are equal modulo 1 KiB those requests meet on the same HBM channel
# (8 % slower at ncrms = 65536).  The library's own buffers (plans, host-array calls) are
# staggered the same way.
STAGGER_BYTES = {"f": 0, "u": 256, "w": 512, "rho": 768}


def empty_staggered(shape, name, dtype=None, device="cuda"):
    """Uninitialised device tensor for array `name` whose base address is
    STAGGER_BYTES[name] modulo 1 KiB (a view into a slightly larger allocation)."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    n = 1
    for x in shape:
        n *= int(x)
    isz = torch.empty((), dtype=dtype).element_size()
    raw = torch.empty(n + 2048 // isz, dtype=dtype, device=device)
    off = (STAGGER_BYTES.get(name, 0) - raw.data_ptr()) % 1024
    return raw[off // isz: off // isz + n].view(tuple(shape))


def _stream_handle(stream):
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    return ctypes.c_void_p(s.cuda_stream)


def _dims_from(f, u):
    """(ncrms, nx, nz, ntracers) from torch tensors in the reversed-axes layout."""
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    if tuple(u.shape) != (nzm, nxp6 - 1, ncrms):
        raise MpdataError(-1, f"u shape {tuple(u.shape)} does not match f {tuple(f.shape)}")
    return ncrms, nxp6 - 6, nzm + 1, nt


def _dev_ptr(t, shape, name, dtype=None):
    import torch
    dtype = torch.float64 if dtype is None else dtype
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise MpdataError(-1, f"{name}: need a contiguous {dtype} device tensor")
    if tuple(t.shape) != tuple(shape):
        raise MpdataError(-1, f"{name}: shape {tuple(t.shape)} != expected {tuple(shape)}")
    return ctypes.c_void_p(t.data_ptr())


def advect_scalar2D(f, u, w, rho, rhow, flux, adz, stream=None):
    """Device-resident `call advect_scalar2D(f,u,w,rho,rhow,flux)` (reference
    :53/:57; adz is host-associated there, :30).  torch float64 device tensors
    (or float32, all seven: the reference's `rp` switch, :12-13) in the
    reversed-axes layout; f and flux are updated in place; asynchronous on
    `stream` (default: torch's current stream)."""
    import torch
    ncrms, nx, nz, nt = _dims_from(f, u)
    sh = shapes(ncrms, nx, nz, nt)
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"f: dtype {f.dtype} is neither float64 nor float32")
    ptrs = [_dev_ptr(t, sh[k], k, f.dtype) for k, t in
            (("f", f), ("u", u), ("w", w), ("rho", rho), ("rhow", rhow), ("adz", adz), ("flux", flux))]
    fn = lib().mpdata_advect_scalar2d_device if f.dtype == torch.float64 else lib().mpdata_advect_scalar2d_f32_device
    _check(fn(ncrms, nx, nz, nt, *ptrs, _stream_handle(stream)))


def stage_shapes(ncrms, nx, nz):
    """torch-side shapes of the reference's temporaries (reference :485-491)."""
    nzm = nz - 1
    return {"uuu": (nzm, nx + 5, ncrms), "www": (nz, nx + 4, ncrms), "mx": (nzm, nx + 2, ncrms),
            "mn": (nzm, nx + 2, ncrms)}


def debug_stages(f, u, w, rho, rhow, flux, adz, tmp, last_stage, stream=None):
    """Stage-by-stage debug mode (include/mpdata_hip.h section 7): run stages 1..last_stage
    unfused; `tmp` = dict of float64 device tensors uuu, www, mx, mn (stage_shapes)."""
    import torch
    ncrms, nx, nz, nt = _dims_from(f, u)
    if nt != 1:
        raise MpdataError(-1, "debug_stages: one tracer")
    sh = shapes(ncrms, nx, nz, 1)
    ptrs = [_dev_ptr(t, sh[k], k, torch.float64) for k, t in
            (("f", f), ("u", u), ("w", w), ("rho", rho), ("rhow", rhow), ("adz", adz), ("flux", flux))]
    ssh = stage_shapes(ncrms, nx, nz)
    tptrs = [_dev_ptr(tmp[k], ssh[k], k, torch.float64) for k in ("uuu", "www", "mx", "mn")]
    _check(lib().mpdata_debug_stages_device(ncrms, nx, nz, int(last_stage), *ptrs, *tptrs,
                                            _stream_handle(stream)))


def _host_ptr(a, name, writable=False, dtype=np.float64):
    if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags["F_CONTIGUOUS"]):
        raise MpdataError(-1, f"{name}: need a Fortran-ordered {np.dtype(dtype).name} numpy array")
    if writable and not a.flags["WRITEABLE"]:
        raise MpdataError(-1, f"{name}: not writable")
    return ctypes.c_void_p(a.ctypes.data)


def _host_dims(f):
    ncrms, nxp6, nzm = f.shape[:3]
    nt = f.shape[3] if f.ndim == 4 else 1
    return ncrms, nxp6 - 6, nzm + 1, nt


def host_shapes(ncrms, nx, nz, ntracers=1):
    """numpy-side (Fortran order, the reference's declarations :479-484, :30) shapes."""
    nzm = nz - 1
    t = (ntracers,) if ntracers > 1 else ()
    return {"adz": (ncrms, nzm), "f": (ncrms, nx + 6, nzm) + t, "u": (ncrms, nx + 5, nzm),
            "w": (ncrms, nx + 4, nz), "rho": (ncrms, nzm), "rhow": (ncrms, nz),
            "flux": (ncrms, nz) + t}


def _host_ptrs(arrs, dims, dt, writable=()):
    """Pointers of host arrays after checking dtype, order AND shape against what the C side
    will copy (a wrongly shaped array would be an out-of-bounds hipMemcpy)."""
    sh = host_shapes(*dims)
    out = []
    for name, a in arrs:
        if a is None:
            out.append(None)
            continue
        p = _host_ptr(a, name, name in writable, dt)
        # a singleton axis (the reference's j = 1) and a trailing tracer axis of 1 are accepted
        got = tuple(x for x in a.shape if x != 1)
        want = tuple(x for x in sh[name] if x != 1)
        if got != want:
            raise MpdataError(-1, f"{name}: shape {tuple(a.shape)} != expected {sh[name]}")
        out.append(p)
    return out


def advect_scalar2D_host(f, u, w, rho, rhow, flux, adz):
    """The drop-in, synchronous call on HOST arrays (numpy, Fortran order,
    reference shapes): H2D + kernel + D2H, like the reference's OpenACC
    routine with its update device/host directives (:107, :241)."""
    ncrms, nx, nz, nt = _host_dims(f)
    dt = np.float32 if isinstance(f, np.ndarray) and f.dtype == np.float32 else np.float64
    fn = lib().mpdata_advect_scalar2d if dt == np.float64 else lib().mpdata_advect_scalar2d_f32
    ptrs = _host_ptrs((("f", f), ("u", u), ("w", w), ("rho", rho), ("rhow", rhow), ("adz", adz), ("flux", flux)),
                      (ncrms, nx, nz, nt), dt, writable=("f", "flux"))
    _check(fn(ncrms, nx, nz, nt, *ptrs))


def release_host_buffers():
    """Free the streams and chunk buffers the host-array call keeps for the calling thread's next call."""
    _check(lib().mpdata_release_host_buffers())


class Plan:
    """Library-owned device state + stream (reference: `!$acc enter data`,
    `update device`, `wait`, `update host`; :105-110, :237-242).  Arrays cross
    the boundary in the reference layout; the plan keeps them in its own layout
    (`layout`: LAYOUT_WAVEMAJOR for nz <= 238 -- fp32: an even ncrms, or any with set_f32_odd_ncrms(1), 3f --,
    include/mpdata_hip.h 3; above 238 levels
    with set_tall_columns(1): as `level_windows` overlapping windows of such a plan, 3e)."""

    def __init__(self, ncrms, nx, nz, ntracers=1, dtype=np.float64, ngpus=None, devices=None):
        """ngpus / devices: a multi-GPU plan (include/mpdata_hip.h section 3b) -- the problem
        is cut into contiguous ncrms blocks, one per GPU; upload scatters, download gathers."""
        self._p = ctypes.c_void_p()
        self._dt = np.dtype(dtype).type
        if self._dt not in (np.float64, np.float32):
            raise MpdataError(-1, f"Plan: dtype {dtype} is neither float64 nor float32")
        self._sfx = "" if self._dt == np.float64 else "_f32"
        self.dims = (int(ncrms), int(nx), int(nz), int(ntracers))
        if ngpus is None and devices is None:
            _check(getattr(lib(), "mpdata_plan_create" + self._sfx)(ncrms, nx, nz, ntracers, ctypes.byref(self._p)))
        else:
            if self._dt != np.float64:
                raise MpdataError(-1, "multi-GPU plans are fp64")
            if devices is not None:
                arr = (ctypes.c_int * len(devices))(*devices)
                _check(lib().mpdata_plan_create_multi_devices(ncrms, nx, nz, ntracers, len(devices), arr,
                                                              ctypes.byref(self._p)))
            else:
                _check(lib().mpdata_plan_create_multi(ncrms, nx, nz, ntracers, int(ngpus), ctypes.byref(self._p)))

    @property
    def ngpus(self):
        return lib().mpdata_plan_ngpus(self._p)

    @property
    def ranks_seen(self):
        """ranks the plan's RCCL communicator reports (ncclCommCount); 0 if the plan has none"""
        return lib().mpdata_plan_ranks_seen(self._p)

    def shards(self):
        """[(device, sl0, nloc)] of the plan's GPUs."""
        out = []
        for g in range(self.ngpus):
            d, a, b = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
            _check(lib().mpdata_plan_shard(self._p, g, ctypes.byref(d), ctypes.byref(a), ctypes.byref(b)))
            out.append((d.value, a.value, b.value))
        return out

    def transfer_stats(self):
        """Multi-GPU plans: seconds and bytes per peer link of the last upload / download."""
        ss, gs = ctypes.c_double(), ctypes.c_double()
        sb, gb, tr = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        _check(lib().mpdata_plan_transfer_stats(self._p, ctypes.byref(ss), ctypes.byref(gs), ctypes.byref(sb),
                                                ctypes.byref(gb), ctypes.byref(tr)))
        return {"scatter_s": ss.value, "gather_s": gs.value, "scatter_bytes_per_peer": sb.value,
                "gather_bytes_per_peer": gb.value, "transport": ("rccl", "p2p", "direct")[tr.value]}

    @property
    def layout(self):
        return lib().mpdata_plan_layout(self._p)

    @property
    def level_windows(self):
        """W: the level windows a column of the plan is cut into (set_tall_columns, nz > 238); 1 for any other plan"""
        return lib().mpdata_plan_level_windows(self._p)

    @property
    def device(self):
        return lib().mpdata_plan_device(self._p)

    @property
    def boundary(self):
        """lateral boundary mode (BOUNDARY_GIVEN, BOUNDARY_PERIODIC)"""
        return lib().mpdata_plan_boundary(self._p)

    def set_boundary(self, mode):
        """BOUNDARY_PERIODIC: every run steps f with halos that are copies of the interior, and f is
        read back wrapped; BOUNDARY_GIVEN (the default): halos are the caller's (mpdata_plan_set_boundary)."""
        _check(lib().mpdata_plan_set_boundary(self._p, int(mode)))

    def upload(self, f, u, w, rho, rhow, adz, flux=None):
        ptrs = _host_ptrs((("f", f), ("u", u), ("w", w), ("rho", rho), ("rhow", rhow), ("adz", adz), ("flux", flux)),
                          self.dims, self._dt)
        _check(getattr(lib(), "mpdata_plan_upload" + self._sfx)(self._p, *ptrs))

    def run(self, first_tracer=None, ntracers=None):
        if first_tracer is None:
            _check(lib().mpdata_plan_run(self._p))
        else:
            _check(lib().mpdata_plan_run_tracers(self._p, int(first_tracer), int(1 if ntracers is None else ntracers)))

    def run_uw(self, u, w, first_tracer=0, ntracers=None):
        """One step on fresh velocities: u, w = reference-layout DEVICE tensors (reversed-axes torch
        layout), f and the rest stay in the plan (mpdata_plan_run_uw)."""
        ncrms, nx, nz, nt = self.dims
        sh = shapes(ncrms, nx, nz, 1)
        pu, pw = _dev_ptr(u, sh["u"], "u", self._tdt()), _dev_ptr(w, sh["w"], "w", self._tdt())
        _check(lib().mpdata_plan_run_uw(self._p, int(first_tracer), int(nt - first_tracer if ntracers is None else ntracers), pu, pw))

    def sync(self):
        _check(lib().mpdata_plan_sync(self._p))

    def download(self, f, flux):
        ptrs = _host_ptrs((("f", f), ("flux", flux)), self.dims, self._dt, writable=("f", "flux"))
        _check(getattr(lib(), "mpdata_plan_download" + self._sfx)(self._p, *ptrs))

    def _tdt(self):
        import torch
        return torch.float64 if self._dt == np.float64 else torch.float32

    def import_device(self, f=None, u=None, w=None, rho=None, rhow=None, adz=None, flux=None, first_tracer=0):
        """Reference-layout DEVICE tensors (reversed-axes torch layout) -> the plan, on the plan's
        stream.  None = keep what the plan has.  f / flux: ([ntr,] nzm, nx+6, ncrms) /
        ([ntr,] nz, ncrms) covering tracers first_tracer .. first_tracer+ntr-1."""
        ncrms, nx, nz, nt = self.dims
        ntr = 1
        for t in (f, flux):
            if t is not None and t.dim() == (4 if t is f else 3):
                ntr = t.shape[0]
        sh = shapes(ncrms, nx, nz, ntr)
        args = []
        for name, t in (("f", f), ("u", u), ("w", w), ("rho", rho), ("rhow", rhow), ("adz", adz), ("flux", flux)):
            args.append(None if t is None else _dev_ptr(t, sh[name], name, self._tdt()))
        _check(lib().mpdata_plan_import_device(self._p, *args, int(first_tracer), int(ntr)))

    def export_device(self, f=None, flux=None, first_tracer=0):
        """The plan's f / flux of tracers first_tracer.. -> reference-layout device tensors."""
        ncrms, nx, nz, nt = self.dims
        ntr = 1
        for t in (f, flux):
            if t is not None and t.dim() == (4 if t is f else 3):
                ntr = t.shape[0]
        sh = shapes(ncrms, nx, nz, ntr)
        pf = None if f is None else _dev_ptr(f, sh["f"], "f", self._tdt())
        pl = None if flux is None else _dev_ptr(flux, sh["flux"], "flux", self._tdt())
        _check(lib().mpdata_plan_export_device(self._p, pf, pl, int(first_tracer), int(ntr)))

    def _block_dims(self, given):
        """(n, ntr) of the block the tensors `given` = [(name, tensor)] describe: n is their common last axis, ntr
        the leading axis of a 4-d f / 3-d flux."""
        n, ntr = None, 1
        for name, t in given:
            if t.dim() < 2:
                raise MpdataError(-1, f"{name}: shape {tuple(t.shape)} is no reference-layout array of a block")
            if n is None:
                n = int(t.shape[-1])
            if name in ("f", "flux") and t.dim() == (4 if name == "f" else 3):
                ntr = int(t.shape[0])
        if n is None:
            raise MpdataError(-1, "block call without an array")
        return n, ntr

    def import_block(self, sl0, f=None, u=None, w=None, rho=None, rhow=None, adz=None, flux=None, first_tracer=0):
        """Reference-layout DEVICE tensors that cover ONLY instances [sl0, sl0+n) -> those instances of the plan
        (mpdata_plan_import_instances_device): exactly the tensors of a problem shapes(n, nx, nz, ntr), n = their last
        axis.  None = keep what the plan has.  The plan must have been filled once as a whole."""
        _, nx, nz, _ = self.dims
        arrs = (("f", f), ("u", u), ("w", w), ("rho", rho), ("rhow", rhow), ("adz", adz), ("flux", flux))
        n, ntr = self._block_dims([(k, t) for k, t in arrs if t is not None])
        sh = shapes(n, nx, nz, ntr)
        args = [None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in arrs]
        _check(lib().mpdata_plan_import_instances_device(self._p, int(sl0), n, *args, int(first_tracer), ntr))

    def export_block(self, sl0, f=None, flux=None, first_tracer=0):
        """Instances [sl0, sl0+n) of the plan's f / flux of tracers first_tracer.. -> reference-layout device tensors
        of a problem of n instances (mpdata_plan_export_instances_device): the slice of what export_device returns."""
        _, nx, nz, _ = self.dims
        arrs = (("f", f), ("flux", flux))
        n, ntr = self._block_dims([(k, t) for k, t in arrs if t is not None])
        sh = shapes(n, nx, nz, ntr)
        pf, pl = (None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in arrs)
        _check(lib().mpdata_plan_export_instances_device(self._p, int(sl0), n, pf, pl, int(first_tracer), ntr))

    def download_block(self, sl0, f, flux):
        """Instances [sl0, sl0+n) of f / flux, all tracers -> HOST arrays (numpy, Fortran order, host_shapes(n, nx, nz,
        ntracers); either may be None), synchronous (mpdata_plan_download_instances)."""
        _, nx, nz, nt = self.dims
        given = [a for a in (f, flux) if a is not None]
        if not given or not isinstance(given[0], np.ndarray) or given[0].ndim < 2:
            raise MpdataError(-1, "download_block: need a numpy array for f or flux")
        n = int(given[0].shape[0])
        ptrs = _host_ptrs((("f", f), ("flux", flux)), (n, nx, nz, nt), self._dt, writable=("f", "flux"))
        _check(getattr(lib(), "mpdata_plan_download_instances" + self._sfx)(self._p, int(sl0), n, *ptrs))

    def _block_n(self, sl0, n):
        """n of a block call: as given, or the rest of the plan from sl0"""
        return self.dims[0] - int(sl0) if n is None else int(n)

    def _block_dev_shape(self, t, n):
        """(shape, ntr) of a device tensor ([ntr,] nzm, n) of a block call: ntr the leading axis of a 3-d tensor"""
        ntr = int(t.shape[0]) if t.dim() == 3 else 1
        return ((ntr,) if t.dim() == 3 else ()) + (self.dims[2] - 1, n), ntr

    def _block_host(self, a, name, want, tracer_axis=False, writable=False):
        """pointer of a host array of a block call after checking dtype, order and shape: `want`, with tracer_axis followed
        by the plan's tracers (one tracer: with or without that axis)"""
        p = _host_ptr(a, name, writable, self._dt)
        nt = self.dims[3]
        full = want + ((nt,) if tracer_axis and nt > 1 else ())
        if tuple(a.shape) != full and not (tracer_axis and nt == 1 and tuple(a.shape) == want + (1,)):
            raise MpdataError(-1, f"{name}: shape {tuple(a.shape)} != expected {full}")
        return p

    @staticmethod
    def _block_ntr(t, ntracers):
        """(ntr, axis) of a block call whose tensor t (or None) may carry a leading tracer axis: ntr = ntracers, or the leading
        axis of a 3-d t (else 1); axis: the shapes of the call carry that axis"""
        lead = t is not None and t.dim() == 3
        ntr = int(ntracers) if ntracers is not None else (int(t.shape[0]) if lead else 1)
        return ntr, lead or ntr != 1

    def level_stats(self, sl0=0, n=None, sum=None, min=None, max=None, first_tracer=0):
        """Horizontal sum / min / max per level of f over the interior columns 1 .. nx, instances [sl0, sl0+n) (default:
        the rest of the plan from sl0) -> reference-layout DEVICE tensors ([ntr,] nzm, n) of the plan's precision, on the
        plan's stream (mpdata_plan_level_stats_device).  None = not wanted; the tracers are first_tracer .. +ntr-1, ntr the
        leading axis of a 3-d tensor.  Changes nothing of the plan."""
        n = self._block_n(sl0, n)
        given = [(k, t) for k, t in (("sum", sum), ("min", min), ("max", max)) if t is not None]
        if not given:
            raise MpdataError(-1, "level_stats: sum, min and max are all None")
        sh, ntr = self._block_dev_shape(given[0][1], n)
        ptrs = [None if t is None else _dev_ptr(t, sh, k, self._tdt()) for k, t in (("sum", sum), ("min", min), ("max", max))]
        _check(lib().mpdata_plan_level_stats_device(self._p, int(sl0), n, *ptrs, int(first_tracer), ntr))

    def level_stats_host(self, sl0=0, n=None, sum=None, min=None, max=None):
        """The same for all tracers into HOST arrays (numpy, Fortran order, (n, nzm[, ntracers]); None = not wanted),
        synchronous (mpdata_plan_level_stats[_f32])."""
        n = self._block_n(sl0, n)
        ptrs = [None if a is None else self._block_host(a, k, (n, self.dims[2] - 1), True, True)
                for k, a in (("sum", sum), ("min", min), ("max", max))]
        if all(p is None for p in ptrs):
            raise MpdataError(-1, "level_stats_host: sum, min and max are all None")
        _check(getattr(lib(), "mpdata_plan_level_stats" + self._sfx)(self._p, int(sl0), n, *ptrs))

    def courant(self, sl0=0, n=None, clev=None, cinst=None):
        """Outflow Courant number of the velocities the plan holds, instances [sl0, sl0+n) (default: the rest of the plan
        from sl0) -> DEVICE tensors of the plan's precision on the plan's stream (mpdata_plan_courant_device): clev (nzm, n)
        the max over the interior columns per level, cinst (n,) its max over the levels.  None = not wanted.  Changes
        nothing of the plan."""
        nz = self.dims[2]
        n = self._block_n(sl0, n)
        if clev is None and cinst is None:
            raise MpdataError(-1, "courant: clev and cinst are both None")
        pl = None if clev is None else _dev_ptr(clev, (nz - 1, n), "clev", self._tdt())
        pi = None if cinst is None else _dev_ptr(cinst, (n,), "cinst", self._tdt())
        _check(lib().mpdata_plan_courant_device(self._p, int(sl0), n, pl, pi))

    def courant_host(self, sl0=0, n=None):
        """The same into new HOST arrays, synchronous (mpdata_plan_courant[_f32]) -> (clev (n, nzm) Fortran order, cinst (n,))"""
        nz = self.dims[2]
        n = self._block_n(sl0, n)
        if n < 1:
            raise MpdataError(-1, f"courant_host: a block of n = {n} instances")
        clev = np.zeros((n, nz - 1), self._dt, order="F")
        cinst = np.zeros((n,), self._dt)
        _check(getattr(lib(), "mpdata_plan_courant" + self._sfx)(self._p, int(sl0), n, ctypes.c_void_p(clev.ctypes.data),
                                                                ctypes.c_void_p(cinst.ctypes.data)))
        return clev, cinst

    def level_add(self, d, sl0=0, n=None, mode=LEVEL_ADD, first_tracer=0):
        """f(sl, i, k, t) += d(sl, k, t) on EVERY column i (halos included) of instances [sl0, sl0+n) (default: the rest of the
        plan from sl0), in place, on the plan's stream (mpdata_plan_level_add_device); mode LEVEL_ADD_CLIP: max(0, .) of the
        sum.  d: a reference-layout DEVICE tensor ([ntr,] nzm, n) of the plan's precision -- the shape of a level_stats
        output; the tracers are first_tracer .. +ntr-1, ntr the leading axis of a 3-d tensor.  d is only read."""
        n = self._block_n(sl0, n)
        sh, ntr = self._block_dev_shape(d, n)
        pd = _dev_ptr(d, sh, "d", self._tdt())
        _check(lib().mpdata_plan_level_add_device(self._p, int(sl0), n, pd, int(mode), int(first_tracer), ntr))

    def level_add_host(self, d, sl0=0, n=None, mode=LEVEL_ADD):
        """The same for all tracers from a HOST array d (numpy, Fortran order, (n, nzm[, ntracers])), synchronous
        (mpdata_plan_level_add[_f32])."""
        n = self._block_n(sl0, n)
        pd = self._block_host(d, "d", (n, self.dims[2] - 1), True)
        _check(getattr(lib(), "mpdata_plan_level_add" + self._sfx)(self._p, int(sl0), n, pd, int(mode)))

    def scale_uw(self, su=None, sw=None, sl0=0, n=None):
        """u(sl, :, :) *= su(sl - sl0), w(sl, :, :) *= sw(sl - sl0) on every column and level of instances [sl0, sl0+n)
        (default: the rest of the plan from sl0), in place, on the plan's stream (mpdata_plan_scale_uw_device).  su, sw:
        DEVICE tensors (n,) of the plan's precision, only read; None leaves that array as it is.  One rounded multiply
        per element; no state of the plan changes."""
        n = self._block_n(sl0, n)
        pu = None if su is None else _dev_ptr(su, (n,), "su", self._tdt())
        pw = None if sw is None else _dev_ptr(sw, (n,), "sw", self._tdt())
        _check(lib().mpdata_plan_scale_uw_device(self._p, int(sl0), n, pu, pw))

    def scale_uw_host(self, su=None, sw=None, sl0=0, n=None):
        """The same from HOST arrays su, sw (numpy, (n,)), synchronous (mpdata_plan_scale_uw[_f32])."""
        n = self._block_n(sl0, n)
        ptrs = [None if a is None else self._block_host(a, name, (n,)) for name, a in (("su", su), ("sw", sw))]
        _check(getattr(lib(), "mpdata_plan_scale_uw" + self._sfx)(self._p, int(sl0), n, *ptrs))

    def column_path(self, path, mass=None, sl0=0, n=None, first_tracer=0, ntracers=None):
        """Mass-weighted column integrals of f (include/mpdata_hip.h 3k): path(sl, i, t) = the sequential sum over k of
        (rho(sl,k) * adz(sl,k)) * f(sl,i,k,t) on the interior columns 1 .. nx, and mass(sl, t) = the sequential sum of path over
        i, instances [sl0, sl0+n) (default: the rest of the plan from sl0) -> reference-layout DEVICE tensors of the plan's
        precision, on the plan's stream (mpdata_plan_column_path_device).  Shapes: column_path_shapes(n, nx, ntr) -- path
        ([ntr,] nx, n), mass ([ntr,] n) or None (skipped).  The tracers are first_tracer .. +ntr-1, ntr = ntracers, or the
        leading axis of a 3-d path (else 1).  Changes nothing of the plan."""
        n = self._block_n(sl0, n)
        nx = self.dims[1]
        ntr, axis = self._block_ntr(path, ntracers)
        sh = column_path_shapes(n, nx, ntr if axis else None)
        pp = _dev_ptr(path, sh["path"], "path", self._tdt())
        pm = None if mass is None else _dev_ptr(mass, sh["mass"], "mass", self._tdt())
        _check(lib().mpdata_plan_column_path_device(self._p, int(sl0), n, pp, pm, int(first_tracer), ntr))

    def column_path_host(self, path, mass=None, sl0=0, n=None):
        """The same for all tracers into HOST arrays (numpy, Fortran order): path (n, nx[, ntracers]), mass (n[, ntracers]) or
        None, synchronous (mpdata_plan_column_path[_f32])."""
        n = self._block_n(sl0, n)
        if path is None:
            raise MpdataError(-1, "column_path_host: path is None")
        ptrs = [None if a is None else self._block_host(a, name, want, True, True)
                for name, a, want in (("path", path, (n, self.dims[1])), ("mass", mass, (n,)))]
        _check(getattr(lib(), "mpdata_plan_column_path" + self._sfx)(self._p, int(sl0), n, *ptrs))

    def diffuse(self, tkh, cx, cz, sb=None, st=None, zflux=None, sl0=0, n=None, first_tracer=0, ntracers=None):
        """Eddy diffusion of f in place (include/mpdata_hip.h 3l) on the interior columns of instances [sl0, sl0+n) (default:
        the rest of the plan from sl0), a Jacobi step from the x- and z-fluxes of the old field, on the plan's stream
        (mpdata_plan_diffuse_device).  Reference-layout DEVICE tensors of the plan's precision, shapes diffuse_shapes(n, nx,
        nz, ntr): tkh (nzm, nx+2, n), cx, cz (nzm, n), sb, st (nx, n) or None (zero flux), zflux ([ntr,] nz, n) or None
        (skipped).  The tracers are first_tracer .. +ntr-1, ntr = ntracers, or the leading axis of a 3-d zflux (else 1).
        Windowed plans: MpdataError (EUNSUPPORTED)."""
        n = self._block_n(sl0, n)
        nx, nz = self.dims[1], self.dims[2]
        ntr, axis = self._block_ntr(zflux, ntracers)
        sh = diffuse_shapes(n, nx, nz, ntr if axis else None)
        ptrs = [None if t is None else _dev_ptr(t, sh[k], k, self._tdt())
                for k, t in (("tkh", tkh), ("cx", cx), ("cz", cz), ("sb", sb), ("st", st), ("zflux", zflux))]
        _check(lib().mpdata_plan_diffuse_device(self._p, int(sl0), n, *ptrs, int(first_tracer), ntr))

    def diffuse_host(self, tkh, cx, cz, sb=None, st=None, zflux=None, sl0=0, n=None):
        """The same for all tracers from HOST arrays (numpy, Fortran order): tkh (n, nx+2, nzm), cx, cz (n, nzm), sb, st
        (n, nx) or None, zflux (n, nz[, ntracers]) or None (written), synchronous (mpdata_plan_diffuse[_f32])."""
        n = self._block_n(sl0, n)
        nx, nz = self.dims[1], self.dims[2]
        ptrs = [None if a is None else self._block_host(a, name, want, out, out)   # (zflux: the tracer axis, and written)
                for name, a, want, out in (("tkh", tkh, (n, nx + 2, nz - 1), False), ("cx", cx, (n, nz - 1), False),
                                           ("cz", cz, (n, nz - 1), False), ("sb", sb, (n, nx), False), ("st", st, (n, nx), False),
                                           ("zflux", zflux, (n, nz), True))]
        _check(getattr(lib(), "mpdata_plan_diffuse" + self._sfx)(self._p, int(sl0), n, *ptrs))

    def subside(self, cb, cc, dsum=None, sl0=0, n=None, first_tracer=0, ntracers=None):
        """Large-scale vertical advection of f in place (include/mpdata_hip.h 3m) on EVERY column (halos included) of
        instances [sl0, sl0+n) (default: the rest of the plan from sl0): f(k) -= cb(k) (f(k) - f(k-1)) + cc(k) (f(k+1) - f(k))
        from the old field, on the plan's stream (mpdata_plan_subside_device).  Reference-layout DEVICE tensors of the
        plan's precision: cb, cc (nzm, n), shared by the tracers; dsum ([ntr,] nzm, n) or None (skipped), the decrement
        summed over the interior columns.  The tracers are first_tracer .. +ntr-1, ntr = ntracers, or the leading axis of a
        3-d dsum (else 1).  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        nzm = self.dims[2] - 1
        ntr, axis = self._block_ntr(dsum, ntracers)
        pb = _dev_ptr(cb, (nzm, n), "cb", self._tdt())
        pc = _dev_ptr(cc, (nzm, n), "cc", self._tdt())
        pd = None if dsum is None else _dev_ptr(dsum, ((ntr,) if axis else ()) + (nzm, n), "dsum", self._tdt())
        _check(lib().mpdata_plan_subside_device(self._p, int(sl0), n, pb, pc, pd, int(first_tracer), ntr))

    def subside_host(self, cb, cc, dsum=None, sl0=0, n=None):
        """The same for all tracers from HOST arrays (numpy, Fortran order): cb, cc (n, nzm), dsum (n, nzm[, ntracers]) or
        None (written), synchronous (mpdata_plan_subside[_f32])."""
        n = self._block_n(sl0, n)
        nzm = self.dims[2] - 1
        ptrs = [self._block_host(cb, "cb", (n, nzm)), self._block_host(cc, "cc", (n, nzm)),
                None if dsum is None else self._block_host(dsum, "dsum", (n, nzm), True, True)]
        _check(getattr(lib(), "mpdata_plan_subside" + self._sfx)(self._p, int(sl0), n, *ptrs))

    def sediment(self, wp, psfc=None, pflux=None, sl0=0, n=None, first_tracer=0, ntracers=None):
        """Sedimentation of f in place (include/mpdata_hip.h 3n) on the interior columns of instances [sl0, sl0+n) (default:
        the rest of the plan from sl0): f(k) -= (wp(k) f(k) - wp(k+1) f(k+1)) / (rho(k) adz(k)) from the old field, nothing
        entering through the top, on the plan's stream (mpdata_plan_sediment_device).  Reference-layout DEVICE tensors of
        the plan's precision, shapes sediment_shapes(n, nx, nz, ntr): wp ([ntr,] nzm, nx, n), one field per tracer, read
        where it lies; psfc ([ntr,] nx, n) or None (skipped), the flux through the surface; pflux ([ntr,] nzm, n) or None
        (skipped), the flux summed over the interior columns.  The tracers are first_tracer .. +ntr-1, ntr = ntracers, or
        the leading axis of a 4-d wp (else 1); psfc and pflux carry that axis exactly when wp does.  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        nx, nz = self.dims[1], self.dims[2]
        # the one tracer-count rule (_block_ntr) on the first tensor given, wp seen without its column axis: the leading
        # axis of any of the three is the tracer axis of all three
        lead = wp[..., 0, :] if wp is not None else (psfc if psfc is not None else pflux)
        ntr, axis = self._block_ntr(lead, ntracers)
        sh = sediment_shapes(n, nx, nz, ntr if axis else None)
        ptrs = [None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in (("wp", wp), ("psfc", psfc), ("pflux", pflux))]
        _check(lib().mpdata_plan_sediment_device(self._p, int(sl0), n, *ptrs, int(first_tracer), ntr))

    def sediment_host(self, wp, psfc=None, pflux=None, sl0=0, n=None):
        """The same for all tracers from HOST arrays (numpy, Fortran order): wp (n, nx, nzm[, ntracers]), psfc (n, nx[,
        ntracers]) or None, pflux (n, nzm[, ntracers]) or None (both written), synchronous (mpdata_plan_sediment[_f32])."""
        n = self._block_n(sl0, n)
        nx, nzm = self.dims[1], self.dims[2] - 1
        ptrs = [None if a is None else self._block_host(a, name, want, True, out)
                for name, a, want, out in (("wp", wp, (n, nx, nzm), False), ("psfc", psfc, (n, nx), True),
                                           ("pflux", pflux, (n, nzm), True))]
        _check(getattr(lib(), "mpdata_plan_sediment" + self._sfx)(self._p, int(sl0), n, *ptrs))

    def vsolve(self, lo, di, up, sl0=0, n=None, first_tracer=0, ntracers=None):
        """Implicit vertical solve of f in place (include/mpdata_hip.h 3o) on the interior columns of instances [sl0, sl0+n)
        (default: the rest of the plan from sl0): f(i,.) := x with lo(k) x(k-1) + di(k) x(k) + up(k) x(k+1) = f(i,k), without
        pivoting, on the plan's stream (mpdata_plan_vsolve_device).  Reference-layout DEVICE tensors of the plan's
        precision, shapes vsolve_shapes(n, nz): lo, di, up (nzm, n), shared by the columns and the tracers.  The tracers
        are first_tracer .. +ntr-1, ntr = ntracers (else 1).  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        ntr, _ = self._block_ntr(None, ntracers)
        sh = vsolve_shapes(n, self.dims[2])
        ptrs = [None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in (("lo", lo), ("di", di), ("up", up))]
        _check(lib().mpdata_plan_vsolve_device(self._p, int(sl0), n, *ptrs, int(first_tracer), ntr))

    def vsolve_host(self, lo, di, up, sl0=0, n=None):
        """The same for all tracers from HOST arrays (numpy, Fortran order): lo, di, up (n, nzm), synchronous
        (mpdata_plan_vsolve[_f32])."""
        n = self._block_n(sl0, n)
        nzm = self.dims[2] - 1
        ptrs = [None if a is None else self._block_host(a, name, (n, nzm)) for name, a in (("lo", lo), ("di", di), ("up", up))]
        _check(getattr(lib(), "mpdata_plan_vsolve" + self._sfx)(self._p, int(sl0), n, *ptrs))

    def vdiffuse(self, tkh, cz, sb=None, st=None, sl0=0, n=None, first_tracer=0, ntracers=None):
        """Implicit vertical diffusion of f with a per-cell diffusivity, in place (include/mpdata_hip.h 3s) on the interior
        columns of instances [sl0, sl0+n) (default: the rest of the plan from sl0): backward Euler of 3l's vertical part,
        the tridiagonal matrix of every column formed from tkh and cz and solved without pivoting, on the plan's stream
        (mpdata_plan_vdiffuse_device).  Reference-layout DEVICE tensors of the plan's precision, shapes vdiffuse_shapes(n,
        nx, nz): tkh (nzm, nx+2, n), 3l's array as it is; cz (nzm, n); sb, st (nx, n) or None (zero flux).  The tracers are
        first_tracer .. +ntr-1, ntr = ntracers (else 1).  Windowed plans: MpdataError (EUNSUPPORTED)."""
        n = self._block_n(sl0, n)
        ntr, _ = self._block_ntr(None, ntracers)
        sh = vdiffuse_shapes(n, self.dims[1], self.dims[2])
        ptrs = [None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in (("tkh", tkh), ("cz", cz), ("sb", sb), ("st", st))]
        _check(lib().mpdata_plan_vdiffuse_device(self._p, int(sl0), n, *ptrs, int(first_tracer), ntr))

    def vdiffuse_host(self, tkh, cz, sb=None, st=None, sl0=0, n=None):
        """The same for all tracers from HOST arrays (numpy, Fortran order): tkh (n, nx+2, nzm), cz (n, nzm), sb, st (n, nx)
        or None, synchronous (mpdata_plan_vdiffuse[_f32])."""
        n = self._block_n(sl0, n)
        nx, nzm = self.dims[1], self.dims[2] - 1
        ptrs = [None if a is None else self._block_host(a, name, want)
                for name, a, want in (("tkh", tkh, (n, nx + 2, nzm)), ("cz", cz, (n, nzm)), ("sb", sb, (n, nx)), ("st", st, (n, nx)))]
        _check(getattr(lib(), "mpdata_plan_vdiffuse" + self._sfx)(self._p, int(sl0), n, *ptrs))

    def cell_add(self, s, c=1.0, mode=CELL_ADD, dsum=None, sl0=0, n=None, first_tracer=0, ntracers=None):
        """Per-cell sources of f in place (include/mpdata_hip.h 3p) on the interior columns of instances [sl0, sl0+n)
        (default: the rest of the plan from sl0): f += c * s, the product and the sum each rounded once; mode CELL_ADD
        (default) or CELL_ADD_CLIP (max(0, .) of the sum), on the plan's stream (mpdata_plan_cell_add_device).
        Reference-layout DEVICE tensors of the plan's precision, shapes cell_add_shapes(n, nx, nz, ntr): s ([ntr,] nzm, nx,
        n), one field per tracer, read where it lies; dsum ([ntr,] nzm, n) or None (skipped), the increment actually
        applied summed over the interior columns.  c is rounded once to the plan's precision.  The tracers are
        first_tracer .. +ntr-1, ntr = ntracers, or the leading axis of a 4-d s (else 1); dsum carries that axis exactly
        when s does.  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        nx, nz = self.dims[1], self.dims[2]
        lead = s[..., 0, :] if s is not None else dsum
        ntr, axis = self._block_ntr(lead, ntracers)
        sh = cell_add_shapes(n, nx, nz, ntr if axis else None)
        ptrs = [None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in (("s", s), ("dsum", dsum))]
        _check(lib().mpdata_plan_cell_add_device(self._p, int(sl0), n, ptrs[0], float(c), int(mode),
                                                 ptrs[1], int(first_tracer), ntr))

    def cell_add_host(self, s, c=1.0, mode=CELL_ADD, dsum=None, sl0=0, n=None):
        """The same for all tracers from HOST arrays (numpy, Fortran order): s (n, nx, nzm[, ntracers]), dsum (n, nzm[,
        ntracers]) or None (written), synchronous (mpdata_plan_cell_add[_f32])."""
        n = self._block_n(sl0, n)
        nx, nzm = self.dims[1], self.dims[2] - 1
        ptrs = [None if a is None else self._block_host(a, name, want, True, out)
                for name, a, want, out in (("s", s, (n, nx, nzm), False), ("dsum", dsum, (n, nzm), True))]
        _check(getattr(lib(), "mpdata_plan_cell_add" + self._sfx)(self._p, int(sl0), n, ptrs[0], float(c),
                                                                  int(mode), ptrs[1]))

    def column_step_device(self, s=None, c=1.0, mode=CELL_ADD, cb=None, cc=None, wp=None, psfc=None, lo=None, di=None, up=None,
                           sl0=0, n=None, first_tracer=0, ntracers=None):
        """The fused column step of f in place (include/mpdata_hip.h 3q) on the interior columns of instances [sl0, sl0+n)
        (default: the rest of the plan from sl0): up to four stages in the fixed order source (s, c, mode: 3p), subside (cb,
        cc: 3m), sediment (wp, psfc: 3n), vsolve (lo, di, up: 3o), a stage present exactly when its tensors are given, with
        one read and one write of f, on the plan's stream (mpdata_plan_column_step_device).  Bit for bit the sequence of
        the single calls on the interior columns; halo columns are not touched and no horizontal sum is formed.
        Reference-layout DEVICE tensors of the plan's precision, shapes column_step_shapes(n, nx, nz, ntr): s, wp ([ntr,]
        nzm, nx, n), psfc ([ntr,] nx, n) or None, cb, cc, lo, di, up (nzm, n).  The tracers are first_tracer .. +ntr-1, ntr
        = ntracers, or the leading axis of a 4-d s or wp (else 1).  Windowed plans are refused (EUNSUPPORTED)."""
        n = self._block_n(sl0, n)
        nx, nz = self.dims[1], self.dims[2]
        lead = s[..., 0, :] if s is not None else (wp[..., 0, :] if wp is not None else psfc)
        ntr, axis = self._block_ntr(lead, ntracers)
        sh = column_step_shapes(n, nx, nz, ntr if axis else None)
        P = {k: None if t is None else _dev_ptr(t, sh[k], k, self._tdt())
             for k, t in (("s", s), ("cb", cb), ("cc", cc), ("wp", wp), ("psfc", psfc), ("lo", lo), ("di", di), ("up", up))}
        _check(lib().mpdata_plan_column_step_device(self._p, int(sl0), n, P["s"], float(c), int(mode), P["cb"], P["cc"], P["wp"],
                                                    P["psfc"], P["lo"], P["di"], P["up"], int(first_tracer), ntr))

    def column_step(self, s=None, c=1.0, mode=CELL_ADD, cb=None, cc=None, wp=None, psfc=None, lo=None, di=None, up=None, sl0=0,
                    n=None):
        """The same for all tracers from HOST arrays (numpy, Fortran order): s, wp (n, nx, nzm[, ntracers]), psfc (n, nx[,
        ntracers]) or None (written), cb, cc, lo, di, up (n, nzm), synchronous (mpdata_plan_column_step[_f32])."""
        n = self._block_n(sl0, n)
        nx, nzm = self.dims[1], self.dims[2] - 1
        P = {name: None if a is None else self._block_host(a, name, want, tr, out)
             for name, a, want, tr, out in (("s", s, (n, nx, nzm), True, False), ("wp", wp, (n, nx, nzm), True, False),
                                            ("psfc", psfc, (n, nx), True, True), ("cb", cb, (n, nzm), False, False),
                                            ("cc", cc, (n, nzm), False, False), ("lo", lo, (n, nzm), False, False),
                                            ("di", di, (n, nzm), False, False), ("up", up, (n, nzm), False, False))}
        _check(getattr(lib(), "mpdata_plan_column_step" + self._sfx)(self._p, int(sl0), n, P["s"], float(c), int(mode), P["cb"],
                                                                     P["cc"], P["wp"], P["psfc"], P["lo"], P["di"], P["up"]))

    def relax(self, c, target=None, mean=None, sl0=0, n=None, first_tracer=0, ntracers=None):
        """Relaxation of f to a level profile in place (include/mpdata_hip.h 3r) on the interior columns of instances [sl0,
        sl0+n) (default: the rest of the plan from sl0): f -= c * (f - m), with m = target, or without a target the
        horizontal mean of f itself (the sum of level_stats over nx, one rounded divide); levels with c == 0 keep every
        bit; on the plan's stream (mpdata_plan_relax_device).  Reference-layout DEVICE tensors of the plan's precision,
        shapes relax_shapes(n, nx, nz, ntr): c (nzm, n), shared by the columns and the tracers; target ([ntr,] nzm, n) or
        None; mean ([ntr,] nzm, n) or None (skipped), written with m in both modes.  The tracers are first_tracer ..
        +ntr-1, ntr = ntracers, or the leading axis of a 3-d target or mean (else 1); target and mean carry that axis
        together.  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        nx, nz = self.dims[1], self.dims[2]
        ntr, axis = self._block_ntr(target if target is not None else mean, ntracers)
        sh = relax_shapes(n, nx, nz, ntr if axis else None)
        ptrs = [None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in (("c", c), ("target", target), ("mean", mean))]
        _check(lib().mpdata_plan_relax_device(self._p, int(sl0), n, *ptrs, int(first_tracer), ntr))

    def relax_host(self, c, target=None, mean=None, sl0=0, n=None):
        """The same for all tracers from HOST arrays (numpy, Fortran order): c (n, nzm), target (n, nzm[, ntracers]) or
        None, mean (n, nzm[, ntracers]) or None (written), synchronous (mpdata_plan_relax[_f32])."""
        n = self._block_n(sl0, n)
        nzm = self.dims[2] - 1
        ptrs = [None if a is None else self._block_host(a, name, (n, nzm), tr, out)
                for name, a, tr, out in (("c", c, False, False), ("target", target, True, False), ("mean", mean, True, True))]
        _check(getattr(lib(), "mpdata_plan_relax" + self._sfx)(self._p, int(sl0), n, *ptrs))

    def nonneg(self, sum=None, nneg=None, sl0=0, n=None, first_tracer=0, ntracers=None):
        """The conservative per-level non-negativity fixer of f in place (include/mpdata_hip.h 3x) on the interior columns
        of instances [sl0, sl0+n) (default: the rest of the plan from sl0): in every row (instance, level, tracer) with a
        negative cell the negative cells become +0 and the others are scaled by s / p, the row's sum over the sum of its
        positive cells (one rounded divide), so that the row keeps its total; a row whose sum is not positive becomes +0
        throughout; a row without a negative cell keeps every bit and is not stored; on the plan's stream
        (mpdata_plan_nonneg_device).  Reference-layout DEVICE tensors of the plan's precision, shapes nonneg_shapes(n,
        nx, nz, ntr): sum ([ntr,] nzm, n) or None, the row sums of the OLD field (the sum of level_stats); nneg ([ntr,] nzm,
        n) or None, the number of negative cells of each row as a real.  The tracers are first_tracer .. +ntr-1, ntr =
        ntracers, or the leading axis of a 3-d sum or nneg (else 1); both carry that axis together; with neither output and
        no ntracers: every tracer from first_tracer on -- Plan.nonneg() fixes the whole plan.  Windowed plans are
        supported."""
        n = self._block_n(sl0, n)
        nx, nz = self.dims[1], self.dims[2]
        if sum is None and nneg is None and ntracers is None:
            ntracers = self.dims[3] - int(first_tracer)
        ntr, axis = self._block_ntr(sum if sum is not None else nneg, ntracers)
        sh = nonneg_shapes(n, nx, nz, ntr if axis else None)
        ptrs = [None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in (("sum", sum), ("nneg", nneg))]
        _check(lib().mpdata_plan_nonneg_device(self._p, int(sl0), n, *ptrs, int(first_tracer), ntr))

    def nonneg_host(self, sum=None, nneg=None, sl0=0, n=None):
        """The same for all tracers into HOST arrays (numpy, Fortran order): sum, nneg (n, nzm[, ntracers]) or None
        (written), synchronous (mpdata_plan_nonneg[_f32])."""
        n = self._block_n(sl0, n)
        nzm = self.dims[2] - 1
        ptrs = [None if a is None else self._block_host(a, name, (n, nzm), True, True) for name, a in (("sum", sum), ("nneg", nneg))]
        _check(getattr(lib(), "mpdata_plan_nonneg" + self._sfx)(self._p, int(sl0), n, *ptrs))

    def satadj(self, th, tq, tn, pres, par, tt=-1, gz=None, mode=0, ncld=None, iters=None, sl0=0, n=None):
        """Saturation adjustment in place (include/mpdata_hip.h 3y) on the interior columns of instances [sl0, sl0+n)
        (default: the rest of the plan from sl0): the condensate (tracer tn, overwritten) and, with tt >= 0, the temperature
        (tracer tt) from the temperature-like tracer th and total water tq, by a Newton iteration per cell on the curves of
        par (a SatadjParams; None reaches the library as a null pointer); mode SATADJ_ICE adds the ice curve and the ramp
        between tmin and tmax; rows with pres == 0 keep every bit of tn and tt; on the plan's stream
        (mpdata_plan_satadj_device).  Reference-layout DEVICE tensors of the plan's precision, shapes satadj_shapes(n, nx,
        nz): pres (nzm, n); gz (nzm, n) or None (T1 = h); ncld, iters (nzm, n) or None (skipped): the cells with
        condensate and the most Newton steps of a row.  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        sh = satadj_shapes(n, self.dims[1], self.dims[2])
        P = {k: None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in (("pres", pres), ("gz", gz), ("ncld", ncld), ("iters", iters))}
        _check(lib().mpdata_plan_satadj_device(self._p, int(sl0), n, int(th), int(tq), int(tn), int(tt), P["pres"], P["gz"],
                                               _satadj_par(par), int(mode), P["ncld"], P["iters"]))

    def satadj_host(self, th, tq, tn, pres, par, tt=-1, gz=None, mode=0, ncld=None, iters=None, sl0=0, n=None):
        """The same from HOST arrays (numpy, Fortran order): pres (n, nzm), gz (n, nzm) or None, ncld, iters (n, nzm) or
        None (written), synchronous (mpdata_plan_satadj[_f32])."""
        n = self._block_n(sl0, n)
        nzm = self.dims[2] - 1
        P = {name: None if a is None else self._block_host(a, name, (n, nzm), False, out)
             for name, a, out in (("pres", pres, False), ("gz", gz, False), ("ncld", ncld, True), ("iters", iters, True))}
        _check(getattr(lib(), "mpdata_plan_satadj" + self._sfx)(self._p, int(sl0), n, int(th), int(tq), int(tn), int(tt), P["pres"],
                                                                P["gz"], _satadj_par(par), int(mode), P["ncld"], P["iters"]))

    def convert(self, src, dst, r, q0=None, y=None, mode=0, dsum=None, sl0=0, n=None):
        """First-order conversion from tracer src to tracer dst in place (include/mpdata_hip.h 3t) on the interior columns
        of instances [sl0, sl0+n) (default: the rest of the plan from sl0): d = r * max(f_src - q0, 0), with mode
        CONVERT_LIMIT capped from above by max(f_src, 0); f_src -= d, f_dst += y * d; levels with r == 0 keep every bit
        of both tracers; on the plan's stream (mpdata_plan_convert_device).  Reference-layout DEVICE tensors of the plan's
        precision, shapes convert_shapes(n, nx, nz): r (nzm, n); q0, y (nzm, n) or None (no threshold, yield 1); dsum
        (nzm, n) or None (skipped), d summed over the interior columns.  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        sh = convert_shapes(n, self.dims[1], self.dims[2])
        ptrs = {k: None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in (("r", r), ("q0", q0), ("y", y), ("dsum", dsum))}
        _check(lib().mpdata_plan_convert_device(self._p, int(sl0), n, int(src), int(dst), ptrs["r"], ptrs["q0"], ptrs["y"], int(mode),
                                                ptrs["dsum"]))

    def convert_host(self, src, dst, r, q0=None, y=None, mode=0, dsum=None, sl0=0, n=None):
        """The same from HOST arrays (numpy, Fortran order): r (n, nzm), q0, y (n, nzm) or None, dsum (n, nzm) or None
        (written), synchronous (mpdata_plan_convert[_f32])."""
        n = self._block_n(sl0, n)
        nzm = self.dims[2] - 1
        ptrs = {name: None if a is None else self._block_host(a, name, (n, nzm), False, out)
                for name, a, out in (("r", r, False), ("q0", q0, False), ("y", y, False), ("dsum", dsum, True))}
        _check(getattr(lib(), "mpdata_plan_convert" + self._sfx)(self._p, int(sl0), n, int(src), int(dst), ptrs["r"], ptrs["q0"],
                                                                 ptrs["y"], int(mode), ptrs["dsum"]))

    def combine(self, dst, src, coef=None, c0=None, mode=0, sum=None, sl0=0, n=None):
        """Linear combination of tracers in place (include/mpdata_hip.h 3z) on the interior columns of instances [sl0,
        sl0+n) (default: the rest of the plan from sl0): f_dst = coef_0 * f_src[0] + coef_1 * f_src[1] + ... + c0, summed in
        the order of src (any sequence of at most COMBINE_MAX ints; sources may repeat and may be dst, which is read old),
        with mode COMBINE_CLIP followed by v = v > 0 ? v : +0; on the plan's stream (mpdata_plan_combine_device).
        Reference-layout DEVICE tensors of the plan's precision, shapes combine_shapes(n, nx, nz, nsrc): coef (nsrc, nzm, n)
        or None (no multiply: one source and no c0 is a bit copy); c0 (nzm, n) or None (required without a source); sum
        (nzm, n) or None (skipped), the new row of dst summed over the interior columns.  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        nsrc, srcp = _src_arg(src)
        sh = combine_shapes(n, self.dims[1], self.dims[2], nsrc)
        P = {k: None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in (("coef", coef), ("c0", c0), ("sum", sum))}
        _check(lib().mpdata_plan_combine_device(self._p, int(sl0), n, int(dst), nsrc, srcp, P["coef"], P["c0"], int(mode), P["sum"]))

    def combine_host(self, dst, src, coef=None, c0=None, mode=0, sum=None, sl0=0, n=None):
        """The same from HOST arrays (numpy, Fortran order): coef (n, nzm, nsrc) or None, c0 (n, nzm) or None, sum (n, nzm)
        or None (written), synchronous (mpdata_plan_combine[_f32])."""
        n = self._block_n(sl0, n)
        nzm = self.dims[2] - 1
        nsrc, srcp = _src_arg(src)
        pc = None
        if coef is not None:
            pc = _host_ptr(coef, "coef", False, self._dt)
            if tuple(coef.shape) != (n, nzm, nsrc):
                raise MpdataError(-1, f"coef: shape {tuple(coef.shape)} != expected {(n, nzm, nsrc)}")
        P = {name: None if a is None else self._block_host(a, name, (n, nzm), False, out) for name, a, out in (("c0", c0, False), ("sum", sum, True))}
        _check(getattr(lib(), "mpdata_plan_combine" + self._sfx)(self._p, int(sl0), n, int(dst), nsrc, srcp, pc, P["c0"], int(mode),
                                                                 P["sum"]))

    def column_scan(self, src, dst, wgt=None, total=None, mode=0, sl0=0, n=None):
        """Running column integral of tracer src into tracer dst, in place (include/mpdata_hip.h 3aa), on the interior columns
        of instances [sl0, sl0+n) (default: the rest of the plan from sl0): p(k) = wgt(k) * f(k, src), s summed from the
        surface upward (mode COLUMN_SCAN_DOWN: from the top downward), f(k, dst) = s including p(k) (COLUMN_SCAN_EXCLUSIVE:
        in front of it); dst == src is the in-place form; on the plan's stream (mpdata_plan_column_scan_device).
        Reference-layout DEVICE tensors of the plan's precision, shapes column_scan_shapes(n, nx, nz): wgt (nzm, n) or None
        (rho * adz of the plan, as column_path); total (nx, n) or None (skipped), the final s.  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        sh = column_scan_shapes(n, self.dims[1], self.dims[2])
        P = {k: None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in (("wgt", wgt), ("total", total))}
        _check(lib().mpdata_plan_column_scan_device(self._p, int(sl0), n, int(src), int(dst), P["wgt"], P["total"], int(mode)))

    def column_scan_host(self, src, dst, wgt=None, total=None, mode=0, sl0=0, n=None):
        """The same from HOST arrays (numpy, Fortran order): wgt (n, nzm) or None, total (n, nx) or None (written),
        synchronous (mpdata_plan_column_scan[_f32])."""
        n = self._block_n(sl0, n)
        P = {name: None if a is None else self._block_host(a, name, want, False, out)
             for name, a, want, out in (("wgt", wgt, (n, self.dims[2] - 1), False), ("total", total, (n, self.dims[1]), True))}
        _check(getattr(lib(), "mpdata_plan_column_scan" + self._sfx)(self._p, int(sl0), n, int(src), int(dst), P["wgt"], P["total"],
                                                                     int(mode)))

    def level_cov(self, ta, tb, cov, ma=None, mb=None, mode=0, mean_a=None, mean_b=None, sl0=0, n=None):
        """Per-level covariance of tracers ta and tb (include/mpdata_hip.h 3u; ta == tb: the variance) over the interior
        columns of instances [sl0, sl0+n) (default: the rest of the plan from sl0): cov = the SUM over i of (a_i - m_a) *
        (b_i - m_b), with m the given profile ma / mb or, without one, the horizontal mean of the row (the sum of
        level_stats over nx, one rounded divide); mode LEVEL_COV_RAW: the sum of a_i * b_i (ma, mb, mean_a, mean_b must be
        None); on the plan's stream (mpdata_plan_level_cov_device).  Reference-layout DEVICE tensors of the plan's precision,
        shapes level_cov_shapes(n, nx, nz), all (nzm, n): cov (written); ma, mb or None; mean_a, mean_b or None (skipped),
        written with the means used.  Changes nothing of the plan.  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        sh = level_cov_shapes(n, self.dims[1], self.dims[2])
        P = {k: None if t is None else _dev_ptr(t, sh[k], k, self._tdt())
             for k, t in (("ma", ma), ("mb", mb), ("cov", cov), ("mean_a", mean_a), ("mean_b", mean_b))}
        _check(lib().mpdata_plan_level_cov_device(self._p, int(sl0), n, int(ta), int(tb), P["ma"], P["mb"], int(mode), P["cov"],
                                                  P["mean_a"], P["mean_b"]))

    def level_cov_host(self, ta, tb, cov, ma=None, mb=None, mode=0, mean_a=None, mean_b=None, sl0=0, n=None):
        """The same with HOST arrays (numpy, Fortran order), all (n, nzm): cov (written), ma, mb or None, mean_a, mean_b or
        None (written), synchronous (mpdata_plan_level_cov[_f32])."""
        n = self._block_n(sl0, n)
        nzm = self.dims[2] - 1
        P = {name: None if a is None else self._block_host(a, name, (n, nzm), False, out)
             for name, a, out in (("ma", ma, False), ("mb", mb, False), ("cov", cov, True), ("mean_a", mean_a, True),
                                  ("mean_b", mean_b, True))}
        _check(getattr(lib(), "mpdata_plan_level_cov" + self._sfx)(self._p, int(sl0), n, int(ta), int(tb), P["ma"], P["mb"], int(mode),
                                                                   P["cov"], P["mean_a"], P["mean_b"]))

    def level_cond(self, tc, lo=None, hi=None, cnt=None, csum=None, first_tracer=0, sl0=0, n=None):
        """Per-level conditional counts and sums (include/mpdata_hip.h 3v) over the interior columns of instances [sl0, sl0+n)
        (default: the rest of the plan from sl0): a column is IN where lo < f(tc) <= hi (a bound that is None does not
        bind; one of the two is needed); cnt = the number of columns that are in, csum[j] = the SUM of tracer first_tracer
        + j over exactly those columns (the caller divides); on the plan's stream (mpdata_plan_level_cond_device).
        Reference-layout DEVICE tensors of the plan's precision, shapes level_cond_shapes(n, nx, nz, ntr): lo, hi, cnt
        (nzm, n), csum (ntr, nzm, n) with ntr its leading axis; cnt or csum may be None (skipped), not both.  Changes
        nothing of the plan.  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        ntr = 0 if csum is None or csum.dim() != 3 else int(csum.shape[0])
        sh = level_cond_shapes(n, self.dims[1], self.dims[2], ntr)
        P = {k: None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in (("lo", lo), ("hi", hi), ("cnt", cnt), ("csum", csum))}
        _check(lib().mpdata_plan_level_cond_device(self._p, int(sl0), n, int(tc), P["lo"], P["hi"], P["cnt"], P["csum"], int(first_tracer),
                                                   ntr))

    def level_cond_host(self, tc, lo=None, hi=None, cnt=None, csum=None, sl0=0, n=None):
        """The same for all tracers with HOST arrays (numpy, Fortran order): lo, hi or None, cnt (written) (n, nzm), csum
        (written) (n, nzm, ntracers); cnt or csum may be None; synchronous (mpdata_plan_level_cond[_f32])."""
        n = self._block_n(sl0, n)
        nzm = self.dims[2] - 1
        P = {name: None if a is None else self._block_host(a, name, (n, nzm), tr, out)
             for name, a, tr, out in (("lo", lo, False, False), ("hi", hi, False, False), ("cnt", cnt, False, True),
                                      ("csum", csum, True, True))}
        _check(getattr(lib(), "mpdata_plan_level_cond" + self._sfx)(self._p, int(sl0), n, int(tc), P["lo"], P["hi"], P["cnt"], P["csum"]))

    def column_cond(self, tc, lo=None, hi=None, kcnt=None, kbot=None, ktop=None, cpath=None, cover=None, mass=None, first_tracer=0,
                    sl0=0, n=None):
        """Per-column conditional level counts, tops and paths (include/mpdata_hip.h 3w) of the interior columns of
        instances [sl0, sl0+n) (default: the rest of the plan from sl0): a level is IN where lo < f(tc) <= hi (a bound that
        is None does not bind; one of the two is needed; lo = +inf shuts a level out: a band of levels); kcnt = the number
        of levels of a column that are in, kbot / ktop = the lowest / highest of them (0: none), cpath[j] = the sum of rho *
        adz * tracer first_tracer + j over exactly those levels, cover = the number of columns with kcnt > 0 (needs kcnt),
        mass[j] = the sum of cpath[j] over the columns (needs cpath); on the plan's stream
        (mpdata_plan_column_cond_device).  Reference-layout DEVICE tensors of the plan's precision, shapes
        column_cond_shapes(n, nx, nz, ntr): lo, hi (nzm, n); kcnt, kbot, ktop (nx, n); cpath (ntr, nx, n) with ntr its
        leading axis; cover (n,); mass (ntr, n); any output may be None (skipped), not all.  Changes nothing of the plan.
        Windowed plans are supported."""
        n = self._block_n(sl0, n)
        ntr = 0 if cpath is None or cpath.dim() != 3 else int(cpath.shape[0])
        sh = column_cond_shapes(n, self.dims[1], self.dims[2], ntr)
        P = {k: None if t is None else _dev_ptr(t, sh[k], k, self._tdt())
             for k, t in (("lo", lo), ("hi", hi), ("kcnt", kcnt), ("kbot", kbot), ("ktop", ktop), ("cpath", cpath), ("cover", cover),
                          ("mass", mass))}
        _check(lib().mpdata_plan_column_cond_device(self._p, int(sl0), n, int(tc), P["lo"], P["hi"], P["kcnt"], P["kbot"], P["ktop"],
                                                    P["cpath"], P["cover"], P["mass"], int(first_tracer), ntr))

    def column_cond_host(self, tc, lo=None, hi=None, kcnt=None, kbot=None, ktop=None, cpath=None, cover=None, mass=None, sl0=0, n=None):
        """The same for all tracers with HOST arrays (numpy, Fortran order): lo, hi (n, nzm) or None; written: kcnt, kbot,
        ktop (n, nx), cpath (n, nx, ntracers), cover (n,), mass (n, ntracers), each or None; synchronous
        (mpdata_plan_column_cond[_f32])."""
        n = self._block_n(sl0, n)
        nx, nzm = self.dims[1], self.dims[2] - 1
        P = {name: None if a is None else self._block_host(a, name, shape, tr, out)
             for name, a, shape, tr, out in (("lo", lo, (n, nzm), False, False), ("hi", hi, (n, nzm), False, False),
                                             ("kcnt", kcnt, (n, nx), False, True), ("kbot", kbot, (n, nx), False, True),
                                             ("ktop", ktop, (n, nx), False, True), ("cpath", cpath, (n, nx), True, True),
                                             ("cover", cover, (n,), False, True), ("mass", mass, (n,), True, True))}
        _check(getattr(lib(), "mpdata_plan_column_cond" + self._sfx)(self._p, int(sl0), n, int(tc), P["lo"], P["hi"], P["kcnt"], P["kbot"],
                                                                    P["ktop"], P["cpath"], P["cover"], P["mass"]))

    def level_hist(self, tc, edges, cnt=None, bsum=None, first_tracer=0, nb=None, sl0=0, n=None):
        """Per-level histograms (include/mpdata_hip.h 3ab) over the interior columns of instances [sl0, sl0+n) (default: the
        rest of the plan from sl0): edges is a HOST sequence of nb + 1 non-decreasing numbers (nb: default len(edges) - 1,
        at most LEVEL_HIST_MAX_BINS); a column is in bin j where edges[j] < f(tc) <= edges[j+1]; cnt[j] = the number of
        columns in bin j, bsum[r, j] = the SUM of tracer first_tracer + r over exactly those columns; on the plan's stream
        (mpdata_plan_level_hist_device).  Reference-layout DEVICE tensors of the plan's precision, shapes
        level_hist_shapes(n, nx, nz, nb, ntr): cnt (nb, nzm, n), bsum (ntr, nb, nzm, n) with ntr its leading axis; cnt or
        bsum may be None (skipped), not both.  Changes nothing of the plan.  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        nb, pe = _edges_arg(edges, nb)
        ntr = 0 if bsum is None or bsum.dim() != 4 else int(bsum.shape[0])
        sh = level_hist_shapes(n, self.dims[1], self.dims[2], nb, ntr)
        P = {k: None if t is None else _dev_ptr(t, sh[k], k, self._tdt()) for k, t in (("cnt", cnt), ("bsum", bsum))}
        _check(lib().mpdata_plan_level_hist_device(self._p, int(sl0), n, int(tc), nb, pe, P["cnt"], P["bsum"], int(first_tracer), ntr))

    def level_hist_host(self, tc, edges, cnt=None, bsum=None, nb=None, sl0=0, n=None):
        """The same for all tracers with HOST arrays (numpy, Fortran order): cnt (written) (n, nzm, nb), bsum (written) (n,
        nzm, nb, ntracers); cnt or bsum may be None; synchronous (mpdata_plan_level_hist[_f32])."""
        n = self._block_n(sl0, n)
        nb, pe = _edges_arg(edges, nb)
        want = (n, self.dims[2] - 1, nb)
        P = {name: None if a is None else self._block_host(a, name, want, tr, True) for name, a, tr in (("cnt", cnt, False), ("bsum", bsum, True))}
        _check(getattr(lib(), "mpdata_plan_level_hist" + self._sfx)(self._p, int(sl0), n, int(tc), nb, pe, P["cnt"], P["bsum"]))

    def level_draft(self, tc=-1, lo=None, hi=None, wup=0.0, wdn=0.0, cnt=None, wsum=None, fsum=None, wfsum=None, first_tracer=0,
                    sl0=0, n=None):
        """Per-level updraft / downdraft sampling (include/mpdata_hip.h 3ac) over the interior columns of instances [sl0,
        sl0+n) (default: the rest of the plan from sl0): with wc = 0.5 * (w(k) + w(k+1)) (+0 above the top) a column where lo
        < f(tc) <= hi (tc = -1: every column; a bound that is None does not bind) is UP (class 0) where wc > wup, DOWN (1)
        where wc < wdn, ENV (2) otherwise; cnt[c] = the columns of class c, wsum[c] = the SUM of wc over them, fsum[j, c] = the
        sum of tracer first_tracer + j, wfsum[j, c] = the sum of wc * tracer; on the plan's stream
        (mpdata_plan_level_draft_device).  wdn <= wup, +-inf allowed.  Reference-layout DEVICE tensors of the plan's
        precision, shapes level_draft_shapes(n, nx, nz, ntr): lo, hi (nzm, n), cnt, wsum (3, nzm, n), fsum, wfsum (ntr, 3,
        nzm, n) with ntr their leading axis; any output may be None (skipped), not all.  The plan must hold w.  Changes
        nothing of the plan.  Windowed plans are supported."""
        n = self._block_n(sl0, n)
        ntr = _draft_ntr(fsum, wfsum)
        sh = level_draft_shapes(n, self.dims[1], self.dims[2], ntr)
        P = {k: None if t is None else _dev_ptr(t, sh[k], k, self._tdt())
             for k, t in (("lo", lo), ("hi", hi), ("cnt", cnt), ("wsum", wsum), ("fsum", fsum), ("wfsum", wfsum))}
        _check(lib().mpdata_plan_level_draft_device(self._p, int(sl0), n, int(tc), P["lo"], P["hi"], float(wup), float(wdn), P["cnt"],
                                                    P["wsum"], P["fsum"], P["wfsum"], int(first_tracer), ntr))

    def level_draft_host(self, tc=-1, lo=None, hi=None, wup=0.0, wdn=0.0, cnt=None, wsum=None, fsum=None, wfsum=None, sl0=0, n=None):
        """The same for all tracers with HOST arrays (numpy, Fortran order): lo, hi or None (n, nzm), cnt, wsum (written) (n,
        nzm, 3), fsum, wfsum (written) (n, nzm, 3, ntracers); any output may be None, not all; synchronous
        (mpdata_plan_level_draft[_f32])."""
        n = self._block_n(sl0, n)
        nzm = self.dims[2] - 1
        P = {name: None if a is None else self._block_host(a, name, want, tr, out)
             for name, a, want, tr, out in (("lo", lo, (n, nzm), False, False), ("hi", hi, (n, nzm), False, False),
                                            ("cnt", cnt, (n, nzm, 3), False, True), ("wsum", wsum, (n, nzm, 3), False, True),
                                            ("fsum", fsum, (n, nzm, 3), True, True), ("wfsum", wfsum, (n, nzm, 3), True, True))}
        _check(getattr(lib(), "mpdata_plan_level_draft" + self._sfx)(self._p, int(sl0), n, int(tc), P["lo"], P["hi"], float(wup),
                                                                     float(wdn), P["cnt"], P["wsum"], P["fsum"], P["wfsum"]))

    def shard_plan(self, g):
        """The single-device plan of GPU g of a multi-GPU plan (mpdata_plan_shard_plan) as a non-owning Plan: device
        import / export and the block calls (shard-local sl0) on the shard where it lives.  Closing the view frees
        nothing; it must not be used after the plan it came from is closed."""
        h = lib().mpdata_plan_shard_plan(self._p, int(g))
        if not h:
            raise MpdataError(-1, f"shard_plan: no shard {g} (the plan has {self.ngpus})")
        nloc = self.shards()[int(g)][2]
        v = Plan.__new__(Plan)
        v._p, v._dt, v._sfx, v._view = ctypes.c_void_p(h), self._dt, self._sfx, True
        v.dims = (int(nloc),) + tuple(self.dims[1:])
        return v

    def set_stream(self, stream=None):
        """Run on a torch stream (default: torch's current stream) from now on."""
        _check(lib().mpdata_plan_set_stream(self._p, _stream_handle(stream)))

    def set_timing(self, on):
        """the plan's own event pair around every run (last_kernel_ms) on / off (mpdata_plan_set_timing)"""
        _check(lib().mpdata_plan_set_timing(self._p, int(bool(on))))

    def last_kernel_ms(self):
        ms = ctypes.c_double()
        _check(lib().mpdata_plan_last_kernel_ms(self._p, ctypes.byref(ms)))
        return ms.value

    def close(self):
        if self._p:
            if not getattr(self, "_view", False):   # (a shard_plan view owns nothing)
                lib().mpdata_plan_destroy(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def periodic_halo(f=None, u=None, w=None, stream=None):
    """Make reference-layout DEVICE tensors (reversed-axes torch layout, float64 or float32, all of one
    dtype) periodic in x, in place: f's columns -2..0, nx+1..nx+3, u's -1, 0, nx+1..nx+3, w's -1, 0,
    nx+1, nx+2 := column 1 + ((i-1) mod nx) (mpdata_periodic_halo_device).  None = left alone."""
    import torch
    given = [(k, t) for k, t in (("f", f), ("u", u), ("w", w)) if t is not None]
    if not given:
        raise MpdataError(-1, "periodic_halo: f, u and w are all None")
    dt = given[0][1].dtype
    if dt not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"periodic_halo: dtype {dt} is neither float64 nor float32")
    nt = 1
    if f is not None:
        nt = f.shape[0] if f.dim() == 4 else 1
        nzm, nxp6, ncrms = f.shape[-3:]
        nx, nz = nxp6 - 6, nzm + 1
    elif u is not None:
        nzm, nxp5, ncrms = u.shape
        nx, nz = nxp5 - 5, nzm + 1
    else:
        nz, nxp4, ncrms = w.shape
        nx = nxp4 - 4
    sh = shapes(ncrms, nx, nz, nt)
    ptrs = [None if t is None else _dev_ptr(t, sh[k], k, dt) for k, t in (("f", f), ("u", u), ("w", w))]
    fn = lib().mpdata_periodic_halo_device if dt == torch.float64 else lib().mpdata_periodic_halo_f32_device
    _check(fn(ncrms, nx, nz, nt, *ptrs, _stream_handle(stream)))


def level_stats(f, sum=None, min=None, max=None, stream=None):
    """Horizontal sum / min / max per level over the interior columns 1 .. nx of a reference-layout DEVICE tensor f
    ([ntr,] nzm, nx+6, ncrms), float64 or float32, into device tensors ([ntr,] nzm, ncrms) of the same dtype (None = not
    wanted), asynchronous on `stream` (mpdata_level_stats_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"level_stats: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() not in (3, 4) or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f")
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    sh = tuple(f.shape[:-3]) + (nzm, ncrms)
    ptrs = [None if t is None else _dev_ptr(t, sh, k, f.dtype) for k, t in (("sum", sum), ("min", min), ("max", max))]
    if all(p is None for p in ptrs):
        raise MpdataError(-1, "level_stats: sum, min and max are all None")
    fn = lib().mpdata_level_stats_device if f.dtype == torch.float64 else lib().mpdata_level_stats_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, pf, *ptrs, _stream_handle(stream)))


def column_path_shapes(n, nx, ntracers=None):
    """Torch shapes (reversed-axes view of the reference layout) of the outputs of a column_path call on n instances:
    path ([ntracers,] nx, n), mass ([ntracers,] n); ntracers None: one tracer without the leading axis."""
    lead = () if ntracers is None else (int(ntracers),)
    return {"path": lead + (int(nx), int(n)), "mass": lead + (int(n),)}


def column_path(f, rho, adz, path, mass=None, stream=None):
    """Mass-weighted column integrals (include/mpdata_hip.h 3k) of a reference-layout DEVICE tensor f ([ntr,] nzm, nx+6,
    ncrms) with rho, adz (nzm, ncrms), float64 or float32, into device tensors path ([ntr,] nx, ncrms) and mass ([ntr,]
    ncrms) of the same dtype (column_path_shapes; mass None: skipped), asynchronous on `stream` (mpdata_column_path_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"column_path: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() not in (3, 4) or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f")
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    if path is None:
        raise MpdataError(-1, "column_path: path is None")
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    pr = _dev_ptr(rho, (nzm, ncrms), "rho", f.dtype)
    pa = _dev_ptr(adz, (nzm, ncrms), "adz", f.dtype)
    sh = column_path_shapes(ncrms, nxp6 - 6, nt if f.dim() == 4 else None)
    pp = _dev_ptr(path, sh["path"], "path", f.dtype)
    pm = None if mass is None else _dev_ptr(mass, sh["mass"], "mass", f.dtype)
    fn = lib().mpdata_column_path_device if f.dtype == torch.float64 else lib().mpdata_column_path_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, pf, pr, pa, pp, pm, _stream_handle(stream)))


def diffuse_shapes(n, nx, nz, ntracers=None):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a diffuse call on n instances: tkh (nzm,
    nx+2, n), cx, cz (nzm, n), sb, st (nx, n), zflux ([ntracers,] nz, n); ntracers None: one tracer without the leading axis."""
    lead = () if ntracers is None else (int(ntracers),)
    n, nx, nz = int(n), int(nx), int(nz)
    return {"tkh": (nz - 1, nx + 2, n), "cx": (nz - 1, n), "cz": (nz - 1, n), "sb": (nx, n), "st": (nx, n), "zflux": lead + (nz, n)}


def diffuse(f, rho, adz, tkh, cx, cz, sb=None, st=None, zflux=None, sl0=0, n=None, stream=None):
    """Eddy diffusion (include/mpdata_hip.h 3l) of instances [sl0, sl0+n) (default: the rest from sl0) of a reference-layout
    DEVICE tensor f ([ntr,] nzm, nx+6, ncrms) with rho, adz (nzm, ncrms), float64 or float32, in place; tkh, cx, cz, sb, st,
    zflux of the same dtype with the shapes of diffuse_shapes(n, nx, nz, ntr) (sb, st, zflux may be None).  Enqueued on
    `stream`; returns when the work is done (mpdata_diffuse_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"diffuse: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() not in (3, 4) or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f")
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    pr = _dev_ptr(rho, (nzm, ncrms), "rho", f.dtype)
    pa = _dev_ptr(adz, (nzm, ncrms), "adz", f.dtype)
    sh = diffuse_shapes(n, nxp6 - 6, nzm + 1, nt if f.dim() == 4 else None)
    ptrs = [None if t is None else _dev_ptr(t, sh[k], k, f.dtype)
            for k, t in (("tkh", tkh), ("cx", cx), ("cz", cz), ("sb", sb), ("st", st), ("zflux", zflux))]
    fn = lib().mpdata_diffuse_device if f.dtype == torch.float64 else lib().mpdata_diffuse_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, pr, pa, *ptrs, _stream_handle(stream)))


def sediment_shapes(n, nx, nz, ntracers=None):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a sediment call on n instances: wp
    ([ntracers,] nzm, nx, n), psfc ([ntracers,] nx, n), pflux ([ntracers,] nzm, n); ntracers None: one tracer without the
    leading axis."""
    lead = () if ntracers is None else (int(ntracers),)
    n, nx, nz = int(n), int(nx), int(nz)
    return {"wp": lead + (nz - 1, nx, n), "psfc": lead + (nx, n), "pflux": lead + (nz - 1, n)}


def sediment(f, rho, adz, wp, psfc=None, pflux=None, sl0=0, n=None, stream=None):
    """Sedimentation (include/mpdata_hip.h 3n) of instances [sl0, sl0+n) (default: the rest from sl0) of a reference-layout
    DEVICE tensor f ([ntr,] nzm, nx+6, ncrms) with rho, adz (nzm, ncrms), float64 or float32, in place; wp, psfc, pflux of
    the same dtype with the shapes of sediment_shapes(n, nx, nz, ntr) (psfc, pflux may be None).  Enqueued on `stream`;
    returns when the work is done (mpdata_sediment_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"sediment: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() not in (3, 4) or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f")
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    pr = _dev_ptr(rho, (nzm, ncrms), "rho", f.dtype)
    pa = _dev_ptr(adz, (nzm, ncrms), "adz", f.dtype)
    sh = sediment_shapes(n, nxp6 - 6, nzm + 1, nt if f.dim() == 4 else None)
    ptrs = [None if t is None else _dev_ptr(t, sh[k], k, f.dtype) for k, t in (("wp", wp), ("psfc", psfc), ("pflux", pflux))]
    fn = lib().mpdata_sediment_device if f.dtype == torch.float64 else lib().mpdata_sediment_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, pr, pa, *ptrs, _stream_handle(stream)))


def cell_add_shapes(n, nx, nz, ntracers=None):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a cell_add call on n instances: s
    ([ntracers,] nzm, nx, n), dsum ([ntracers,] nzm, n); ntracers None: one tracer without the leading axis."""
    lead = () if ntracers is None else (int(ntracers),)
    n, nx, nz = int(n), int(nx), int(nz)
    return {"s": lead + (nz - 1, nx, n), "dsum": lead + (nz - 1, n)}


def cell_add(f, s, c=1.0, mode=CELL_ADD, dsum=None, sl0=0, n=None, stream=None):
    """Per-cell sources (include/mpdata_hip.h 3p) of instances [sl0, sl0+n) (default: the rest from sl0) of a
    reference-layout DEVICE tensor f ([ntr,] nzm, nx+6, ncrms), float64 or float32, in place: f += c * s on the interior
    columns, mode CELL_ADD (default) or CELL_ADD_CLIP; s, dsum of the same dtype with the shapes of cell_add_shapes(n, nx,
    nz, ntr) (dsum may be None).  Asynchronous on `stream` (mpdata_cell_add_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"cell_add: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() not in (3, 4) or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f")
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    sh = cell_add_shapes(n, nxp6 - 6, nzm + 1, nt if f.dim() == 4 else None)
    ptrs = [None if t is None else _dev_ptr(t, sh[k], k, f.dtype) for k, t in (("s", s), ("dsum", dsum))]
    fn = lib().mpdata_cell_add_device if f.dtype == torch.float64 else lib().mpdata_cell_add_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, ptrs[0], float(c), int(mode), ptrs[1],
              _stream_handle(stream)))


def column_step_shapes(n, nx, nz, ntracers=None):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a column_step call on n instances: s, wp
    ([ntracers,] nzm, nx, n), psfc ([ntracers,] nx, n), cb, cc, lo, di, up (nzm, n); ntracers None: one tracer without the
    leading axis."""
    lead = () if ntracers is None else (int(ntracers),)
    n, nx, nz = int(n), int(nx), int(nz)
    sh = {k: (nz - 1, n) for k in ("cb", "cc", "lo", "di", "up")}
    sh.update({"s": lead + (nz - 1, nx, n), "wp": lead + (nz - 1, nx, n), "psfc": lead + (nx, n)})
    return sh


def column_step_device(f, rho=None, adz=None, s=None, c=1.0, mode=CELL_ADD, cb=None, cc=None, wp=None, psfc=None, lo=None, di=None,
                       up=None, sl0=0, n=None, stream=None):
    """The fused column step (include/mpdata_hip.h 3q) of instances [sl0, sl0+n) (default: the rest from sl0) of a
    reference-layout DEVICE tensor f ([ntr,] nzm, nx+6, ncrms), float64 or float32, in place, with rho, adz (nzm, ncrms)
    required only with wp; the stages' tensors of the same dtype with the shapes of column_step_shapes(n, nx, nz, ntr), a
    stage present exactly when its tensors are given.  Enqueued on `stream`; with lo, di, up the call returns when the work
    is done (mpdata_column_step_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"column_step: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() not in (3, 4) or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f")
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    pr = None if rho is None else _dev_ptr(rho, (nzm, ncrms), "rho", f.dtype)
    pa = None if adz is None else _dev_ptr(adz, (nzm, ncrms), "adz", f.dtype)
    sh = column_step_shapes(n, nxp6 - 6, nzm + 1, nt if f.dim() == 4 else None)
    P = {k: None if t is None else _dev_ptr(t, sh[k], k, f.dtype)
         for k, t in (("s", s), ("cb", cb), ("cc", cc), ("wp", wp), ("psfc", psfc), ("lo", lo), ("di", di), ("up", up))}
    fn = lib().mpdata_column_step_device if f.dtype == torch.float64 else lib().mpdata_column_step_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, pr, pa, P["s"], float(c), int(mode), P["cb"], P["cc"], P["wp"],
              P["psfc"], P["lo"], P["di"], P["up"], _stream_handle(stream)))


def relax_shapes(n, nx, nz, ntracers=None):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a relax call on n instances: c (nzm, n),
    target and mean ([ntracers,] nzm, n); ntracers None: one tracer without the leading axis.  (nx is taken as the other
    shape functions take it; no array of the call has a column axis.)"""
    lead = () if ntracers is None else (int(ntracers),)
    n, nx, nz = int(n), int(nx), int(nz)
    return {"c": (nz - 1, n), "target": lead + (nz - 1, n), "mean": lead + (nz - 1, n)}


def relax(f, c, target=None, mean=None, sl0=0, n=None, stream=None):
    """Relaxation to a level profile (include/mpdata_hip.h 3r) of instances [sl0, sl0+n) (default: the rest from sl0) of a
    reference-layout DEVICE tensor f ([ntr,] nzm, nx+6, ncrms), float64 or float32, in place: f -= c * (f - m) on the
    interior columns, m = target or, without one, the horizontal mean of f; c, target, mean of the same dtype with the
    shapes of relax_shapes(n, nx, nz, ntr) (target, mean may be None).  Asynchronous on `stream` (mpdata_relax_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"relax: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() not in (3, 4) or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f")
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    sh = relax_shapes(n, nxp6 - 6, nzm + 1, nt if f.dim() == 4 else None)
    ptrs = [None if t is None else _dev_ptr(t, sh[k], k, f.dtype) for k, t in (("c", c), ("target", target), ("mean", mean))]
    fn = lib().mpdata_relax_device if f.dtype == torch.float64 else lib().mpdata_relax_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, *ptrs, _stream_handle(stream)))


def nonneg_shapes(n, nx, nz, ntracers=None):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a nonneg call on n instances: sum and
    nneg ([ntracers,] nzm, n); ntracers None: one tracer without the leading axis.  (nx is taken as the other shape
    functions take it; no array of the call has a column axis.)"""
    lead = () if ntracers is None else (int(ntracers),)
    n, nx, nz = int(n), int(nx), int(nz)
    return {"sum": lead + (nz - 1, n), "nneg": lead + (nz - 1, n)}


def nonneg(f, sum=None, nneg=None, sl0=0, n=None, stream=None):
    """The conservative per-level non-negativity fixer (include/mpdata_hip.h 3x) of instances [sl0, sl0+n) (default: the
    rest from sl0) of a reference-layout DEVICE tensor f ([ntr,] nzm, nx+6, ncrms), float64 or float32, in place: rows of
    the interior columns with a negative cell get their negative cells zeroed and the others scaled so that the row keeps
    its sum (all +0 where the sum is not positive); sum, nneg of the same dtype with the shapes of nonneg_shapes(n, nx,
    nz, ntr), each may be None.  Asynchronous on `stream` (mpdata_nonneg_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"nonneg: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() not in (3, 4) or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f")
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    sh = nonneg_shapes(n, nxp6 - 6, nzm + 1, nt if f.dim() == 4 else None)
    ptrs = [None if t is None else _dev_ptr(t, sh[k], k, f.dtype) for k, t in (("sum", sum), ("nneg", nneg))]
    fn = lib().mpdata_nonneg_device if f.dtype == torch.float64 else lib().mpdata_nonneg_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, *ptrs, _stream_handle(stream)))


def _satadj_par(par):
    """the par argument of a satadj call: a SatadjParams by reference, None as the null pointer"""
    if par is None:
        return None
    if not isinstance(par, SatadjParams):
        raise MpdataError(-1, f"par: {type(par).__name__} is no SatadjParams")
    return ctypes.byref(par)


def satadj_shapes(n, nx, nz):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a satadj call on n instances: pres, gz,
    ncld, iters (nzm, n).  (nx is taken as the other shape functions take it; no array of the call has a column axis.)"""
    n, nx, nz = int(n), int(nx), int(nz)
    return {k: (nz - 1, n) for k in ("pres", "gz", "ncld", "iters")}


def satadj(f, th, tq, tn, pres, par, tt=-1, gz=None, mode=0, ncld=None, iters=None, sl0=0, n=None, stream=None):
    """Saturation adjustment (include/mpdata_hip.h 3y) of instances [sl0, sl0+n) (default: the rest from sl0) of a
    reference-layout DEVICE tensor f (ntr, nzm, nx+6, ncrms), float64 or float32, in place: tracer tn becomes the condensate
    and, with tt >= 0, tracer tt the temperature diagnosed from tracers th and tq on the interior columns; par a
    SatadjParams, mode 0 or SATADJ_ICE; pres, gz, ncld, iters of the same dtype with the shapes of satadj_shapes(n, nx, nz)
    (gz, ncld, iters may be None).  Asynchronous on `stream` (mpdata_satadj_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"satadj: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() != 4 or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f with a tracer axis")
    nt, nzm, nxp6, ncrms = f.shape
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    sh = satadj_shapes(n, nxp6 - 6, nzm + 1)
    P = {k: None if t is None else _dev_ptr(t, sh[k], k, f.dtype) for k, t in (("pres", pres), ("gz", gz), ("ncld", ncld), ("iters", iters))}
    fn = lib().mpdata_satadj_device if f.dtype == torch.float64 else lib().mpdata_satadj_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, int(th), int(tq), int(tn), int(tt), P["pres"], P["gz"], _satadj_par(par),
              int(mode), P["ncld"], P["iters"], _stream_handle(stream)))


def convert_shapes(n, nx, nz):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a convert call on n instances: r, q0, y,
    dsum (nzm, n).  (nx is taken as the other shape functions take it; no array of the call has a column axis.)"""
    n, nx, nz = int(n), int(nx), int(nz)
    return {k: (nz - 1, n) for k in ("r", "q0", "y", "dsum")}


def convert(f, src, dst, r, q0=None, y=None, mode=0, dsum=None, sl0=0, n=None, stream=None):
    """First-order conversion from tracer src to tracer dst (include/mpdata_hip.h 3t) of instances [sl0, sl0+n) (default:
    the rest from sl0) of a reference-layout DEVICE tensor f (ntr, nzm, nx+6, ncrms), float64 or float32, in place: d = r *
    max(f_src - q0, 0), with mode CONVERT_LIMIT capped by max(f_src, 0); f_src -= d, f_dst += y * d on the interior columns;
    r, q0, y, dsum of the same dtype with the shapes of convert_shapes(n, nx, nz) (q0, y, dsum may be None).  Asynchronous
    on `stream` (mpdata_convert_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"convert: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() != 4 or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f with a tracer axis")
    nt, nzm, nxp6, ncrms = f.shape
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    sh = convert_shapes(n, nxp6 - 6, nzm + 1)
    P = {k: None if t is None else _dev_ptr(t, sh[k], k, f.dtype) for k, t in (("r", r), ("q0", q0), ("y", y), ("dsum", dsum))}
    fn = lib().mpdata_convert_device if f.dtype == torch.float64 else lib().mpdata_convert_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, int(src), int(dst), P["r"], P["q0"], P["y"], int(mode), P["dsum"],
              _stream_handle(stream)))


def _edges_arg(edges, nb=None):
    """the (nb, edges) arguments of a level_hist call: any sequence of numbers -> (nb, a C array of double); None reaches the
    library as a null pointer (nb as given, or 0); nb defaults to len(edges) - 1 and may not ask for more edges than given"""
    if edges is None:
        return (0 if nb is None else int(nb)), None
    e = [float(x) for x in edges]
    nb = len(e) - 1 if nb is None else int(nb)
    if nb + 1 > len(e):
        raise MpdataError(-1, f"edges: {len(e)} values are fewer than nb + 1 = {nb + 1}")
    return nb, (ctypes.cast((ctypes.c_double * len(e))(*e), ctypes.c_void_p) if e else None)


def level_hist_shapes(n, nx, nz, nb, ntr=1):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a level_hist call on n instances, nb bins
    and ntr value tracers: cnt (nb, nzm, n), bsum (ntr, nb, nzm, n).  (nx is taken as the other shape functions take it; no
    array of the call has a column axis.)"""
    n, nx, nz, nb, ntr = int(n), int(nx), int(nz), int(nb), int(ntr)
    return {"cnt": (nb, nz - 1, n), "bsum": (ntr, nb, nz - 1, n)}


def level_hist(f, tc, edges, cnt=None, bsum=None, first_tracer=0, nb=None, sl0=0, n=None, stream=None):
    """Per-level histograms (include/mpdata_hip.h 3ab) of instances [sl0, sl0+n) (default: the rest from sl0) of a
    reference-layout DEVICE tensor f (ntr, nzm, nx+6, ncrms), float64 or float32, which is only read: a column is in bin j
    where edges[j] < f[tc] <= edges[j+1] (edges: a HOST sequence of nb + 1 non-decreasing numbers); cnt[j] = the number of
    interior columns in bin j, bsum[r, j] = the sum of tracer first_tracer + r over them.  cnt, bsum of the same dtype with
    the shapes of level_hist_shapes(n, nx, nz, nb, ntr), ntr the leading axis of bsum (cnt or bsum may be None).
    Asynchronous on `stream` (mpdata_level_hist_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"level_hist: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() != 4 or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f with a tracer axis")
    nt, nzm, nxp6, ncrms = f.shape
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    nb, pe = _edges_arg(edges, nb)
    ntr = 0 if bsum is None or bsum.dim() != 4 else int(bsum.shape[0])
    sh = level_hist_shapes(n, nxp6 - 6, nzm + 1, nb, ntr)
    P = {k: None if t is None else _dev_ptr(t, sh[k], k, f.dtype) for k, t in (("cnt", cnt), ("bsum", bsum))}
    fn = lib().mpdata_level_hist_device if f.dtype == torch.float64 else lib().mpdata_level_hist_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, int(tc), nb, pe, P["cnt"], P["bsum"], int(first_tracer), ntr,
              _stream_handle(stream)))


def _draft_ntr(fsum, wfsum):
    """the value tracers of a level_draft call: the leading axis of fsum, else of wfsum (0: neither given, or no 4-d tensor;
    a wfsum of another count than fsum fails the shape check)"""
    for t in (fsum, wfsum):
        if t is not None:
            return int(t.shape[0]) if t.dim() == 4 else 0
    return 0


def level_draft_shapes(n, nx, nz, ntr=1):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a level_draft call on n instances and ntr
    value tracers: lo, hi (nzm, n), cnt, wsum (3, nzm, n), fsum, wfsum (ntr, 3, nzm, n); the class axis is UP, DOWN, ENV.
    (nx is taken as the other shape functions take it; no array of the call has a column axis.)"""
    n, nx, nz, ntr = int(n), int(nx), int(nz), int(ntr)
    return {"lo": (nz - 1, n), "hi": (nz - 1, n), "cnt": (3, nz - 1, n), "wsum": (3, nz - 1, n), "fsum": (ntr, 3, nz - 1, n),
            "wfsum": (ntr, 3, nz - 1, n)}


def level_draft(f, w, tc=-1, lo=None, hi=None, wup=0.0, wdn=0.0, cnt=None, wsum=None, fsum=None, wfsum=None, first_tracer=0, sl0=0,
                n=None, stream=None):
    """Per-level updraft / downdraft sampling (include/mpdata_hip.h 3ac) of instances [sl0, sl0+n) (default: the rest from
    sl0) of reference-layout DEVICE tensors f (ntr, nzm, nx+6, ncrms) and w (nz, nx+4, ncrms), float64 or float32, which are
    only read: with wc = 0.5 * (w[k] + w[k+1]) (+0 above the top; w[nz-1] is never read) a column where lo < f[tc] <= hi (tc =
    -1: every column) is UP where wc > wup, DOWN where wc < wdn, ENV otherwise; cnt, wsum, fsum, wfsum per class as
    Plan.level_draft, of the same dtype with the shapes of level_draft_shapes(n, nx, nz, ntr).  f may be None where tc < 0 and
    neither fsum nor wfsum is given.  Asynchronous on `stream` (mpdata_level_draft_device)."""
    import torch
    if w is None or w.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, "level_draft: w is None or neither float64 nor float32")
    if w.dim() != 3 or w.shape[-2] < 5 or w.shape[0] < 2:
        raise MpdataError(-1, f"w: shape {tuple(w.shape)} is no reference-layout w")
    nz, nxp4, ncrms = w.shape
    nt = 1
    pf = None
    if f is not None:
        if f.dim() != 4 or tuple(f.shape[1:]) != (nz - 1, nxp4 + 2, ncrms):
            raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f with a tracer axis beside w {tuple(w.shape)}")
        nt = int(f.shape[0])
        pf = _dev_ptr(f, tuple(f.shape), "f", w.dtype)
    n = ncrms - int(sl0) if n is None else int(n)
    pw = _dev_ptr(w, tuple(w.shape), "w", w.dtype)
    ntr = _draft_ntr(fsum, wfsum)
    sh = level_draft_shapes(n, nxp4 - 4, nz, ntr)
    P = {k: None if t is None else _dev_ptr(t, sh[k], k, w.dtype)
         for k, t in (("lo", lo), ("hi", hi), ("cnt", cnt), ("wsum", wsum), ("fsum", fsum), ("wfsum", wfsum))}
    fn = lib().mpdata_level_draft_device if w.dtype == torch.float64 else lib().mpdata_level_draft_f32_device
    _check(fn(ncrms, nxp4 - 4, nz, nt, int(sl0), n, pf, pw, int(tc), P["lo"], P["hi"], float(wup), float(wdn), P["cnt"], P["wsum"],
              P["fsum"], P["wfsum"], int(first_tracer), ntr, _stream_handle(stream)))


def _src_arg(src):
    """the src argument of a combine call: any sequence of ints -> (nsrc, a C array of int or None for an empty one)"""
    src = [int(t) for t in src]
    return len(src), (ctypes.cast((ctypes.c_int * len(src))(*src), ctypes.c_void_p) if src else None)


def combine_shapes(n, nx, nz, nsrc):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a combine call on n instances and nsrc
    sources: coef (nsrc, nzm, n); c0, sum (nzm, n).  (nx is taken as the other shape functions take it; no array of the
    call has a column axis.)"""
    n, nx, nz, nsrc = int(n), int(nx), int(nz), int(nsrc)
    return {"coef": (nsrc, nz - 1, n), "c0": (nz - 1, n), "sum": (nz - 1, n)}


def combine(f, dst, src, coef=None, c0=None, mode=0, sum=None, sl0=0, n=None, stream=None):
    """Linear combination of tracers (include/mpdata_hip.h 3z) of instances [sl0, sl0+n) (default: the rest from sl0) of a
    reference-layout DEVICE tensor f (ntr, nzm, nx+6, ncrms), float64 or float32, in place: f_dst = coef_0 * f_src[0] + ... +
    c0 on the interior columns, in the order of src (any sequence of at most COMBINE_MAX ints), with mode COMBINE_CLIP
    clipped at zero; coef, c0, sum of the same dtype with the shapes of combine_shapes(n, nx, nz, nsrc) (each may be None;
    c0 is required without a source).  Asynchronous on `stream` (mpdata_combine_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"combine: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() != 4 or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f with a tracer axis")
    nt, nzm, nxp6, ncrms = f.shape
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    nsrc, srcp = _src_arg(src)
    sh = combine_shapes(n, nxp6 - 6, nzm + 1, nsrc)
    P = {k: None if t is None else _dev_ptr(t, sh[k], k, f.dtype) for k, t in (("coef", coef), ("c0", c0), ("sum", sum))}
    fn = lib().mpdata_combine_device if f.dtype == torch.float64 else lib().mpdata_combine_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, int(dst), nsrc, srcp, P["coef"], P["c0"], int(mode), P["sum"],
              _stream_handle(stream)))


def column_scan_shapes(n, nx, nz):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a column_scan call on n instances: wgt
    (nzm, n), total (nx, n)."""
    n, nx, nz = int(n), int(nx), int(nz)
    return {"wgt": (nz - 1, n), "total": (nx, n)}


def column_scan(f, src, dst, wgt, total=None, mode=0, sl0=0, n=None, stream=None):
    """Running column integral (include/mpdata_hip.h 3aa) of tracer src into tracer dst of instances [sl0, sl0+n) (default:
    the rest from sl0) of a reference-layout DEVICE tensor f (ntr, nzm, nx+6, ncrms), float64 or float32, in place: f(k, dst)
    = the sum of wgt * f(src) from the surface up to k (mode COLUMN_SCAN_DOWN: from the top down to it; COLUMN_SCAN_EXCLUSIVE:
    without level k itself) on the interior columns; wgt (required) and total (or None) of the same dtype with the shapes of
    column_scan_shapes(n, nx, nz).  Asynchronous on `stream` (mpdata_column_scan_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"column_scan: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() != 4 or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f with a tracer axis")
    nt, nzm, nxp6, ncrms = f.shape
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    sh = column_scan_shapes(n, nxp6 - 6, nzm + 1)
    P = {k: None if t is None else _dev_ptr(t, sh[k], k, f.dtype) for k, t in (("wgt", wgt), ("total", total))}
    fn = lib().mpdata_column_scan_device if f.dtype == torch.float64 else lib().mpdata_column_scan_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, int(src), int(dst), P["wgt"], P["total"], int(mode), _stream_handle(stream)))


def level_cov_shapes(n, nx, nz):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a level_cov call on n instances: ma, mb,
    cov, mean_a, mean_b (nzm, n).  (nx is taken as the other shape functions take it; no array of the call has a column
    axis.)"""
    n, nx, nz = int(n), int(nx), int(nz)
    return {k: (nz - 1, n) for k in ("ma", "mb", "cov", "mean_a", "mean_b")}


def level_cov(f, ta, tb, cov, ma=None, mb=None, mode=0, mean_a=None, mean_b=None, sl0=0, n=None, stream=None):
    """Per-level covariance of tracers ta and tb (include/mpdata_hip.h 3u) of instances [sl0, sl0+n) (default: the rest
    from sl0) of a reference-layout DEVICE tensor f (ntr, nzm, nx+6, ncrms), float64 or float32, which is only read: cov =
    the sum over the interior columns of (a_i - m_a) * (b_i - m_b), m = ma / mb or the horizontal mean of the row; mode
    LEVEL_COV_RAW: the sum of a_i * b_i.  cov, ma, mb, mean_a, mean_b of the same dtype with the shapes of
    level_cov_shapes(n, nx, nz) (all but cov may be None).  Asynchronous on `stream` (mpdata_level_cov_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"level_cov: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() != 4 or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f with a tracer axis")
    nt, nzm, nxp6, ncrms = f.shape
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    sh = level_cov_shapes(n, nxp6 - 6, nzm + 1)
    P = {k: None if t is None else _dev_ptr(t, sh[k], k, f.dtype)
         for k, t in (("ma", ma), ("mb", mb), ("cov", cov), ("mean_a", mean_a), ("mean_b", mean_b))}
    fn = lib().mpdata_level_cov_device if f.dtype == torch.float64 else lib().mpdata_level_cov_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, int(ta), int(tb), P["ma"], P["mb"], int(mode), P["cov"], P["mean_a"],
              P["mean_b"], _stream_handle(stream)))


def level_cond_shapes(n, nx, nz, ntr=1):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a level_cond call on n instances and ntr
    value tracers: lo, hi, cnt (nzm, n), csum (ntr, nzm, n).  (nx is taken as the other shape functions take it; no array
    of the call has a column axis.)"""
    n, nx, nz, ntr = int(n), int(nx), int(nz), int(ntr)
    return {"lo": (nz - 1, n), "hi": (nz - 1, n), "cnt": (nz - 1, n), "csum": (ntr, nz - 1, n)}


def level_cond(f, tc, lo=None, hi=None, cnt=None, csum=None, first_tracer=0, sl0=0, n=None, stream=None):
    """Per-level conditional counts and sums (include/mpdata_hip.h 3v) of instances [sl0, sl0+n) (default: the rest from
    sl0) of a reference-layout DEVICE tensor f (ntr, nzm, nx+6, ncrms), float64 or float32, which is only read: a column is
    in where lo < f[tc] <= hi; cnt = the number of interior columns that are in, csum[j] = the sum of tracer first_tracer +
    j over them.  lo, hi, cnt, csum of the same dtype with the shapes of level_cond_shapes(n, nx, nz, ntr), ntr the leading
    axis of csum (lo or hi, and cnt or csum, may be None).  Asynchronous on `stream` (mpdata_level_cond_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"level_cond: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() != 4 or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f with a tracer axis")
    nt, nzm, nxp6, ncrms = f.shape
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    ntr = 0 if csum is None or csum.dim() != 3 else int(csum.shape[0])
    sh = level_cond_shapes(n, nxp6 - 6, nzm + 1, ntr)
    P = {k: None if t is None else _dev_ptr(t, sh[k], k, f.dtype) for k, t in (("lo", lo), ("hi", hi), ("cnt", cnt), ("csum", csum))}
    fn = lib().mpdata_level_cond_device if f.dtype == torch.float64 else lib().mpdata_level_cond_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, int(tc), P["lo"], P["hi"], P["cnt"], P["csum"], int(first_tracer), ntr,
              _stream_handle(stream)))


def column_cond_shapes(n, nx, nz, ntr=1):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a column_cond call on n instances and
    ntr value tracers: lo, hi (nzm, n); kcnt, kbot, ktop (nx, n); cpath (ntr, nx, n); cover (n,); mass (ntr, n)."""
    n, nx, nz, ntr = int(n), int(nx), int(nz), int(ntr)
    return {"lo": (nz - 1, n), "hi": (nz - 1, n), "kcnt": (nx, n), "kbot": (nx, n), "ktop": (nx, n), "cpath": (ntr, nx, n),
            "cover": (n,), "mass": (ntr, n)}


def column_cond(f, rho, adz, tc, lo=None, hi=None, kcnt=None, kbot=None, ktop=None, cpath=None, cover=None, mass=None, first_tracer=0,
                sl0=0, n=None, stream=None):
    """Per-column conditional level counts, tops and paths (include/mpdata_hip.h 3w) of instances [sl0, sl0+n) (default: the
    rest from sl0) of reference-layout DEVICE tensors f (ntr, nzm, nx+6, ncrms), rho, adz (nzm, ncrms), float64 or float32,
    which are only read: a level is in where lo < f[tc] <= hi; kcnt = the levels of a column that are in, kbot / ktop = the
    lowest / highest of them, cpath[j] = the sum of rho * adz * tracer first_tracer + j over them, cover = the columns with
    kcnt > 0, mass[j] = the sum of cpath[j] over the columns.  lo, hi and the outputs of the same dtype with the shapes of
    column_cond_shapes(n, nx, nz, ntr), ntr the leading axis of cpath (lo or hi, and all outputs but one, may be None).
    Asynchronous on `stream` (mpdata_column_cond_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"column_cond: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() != 4 or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f with a tracer axis")
    nt, nzm, nxp6, ncrms = f.shape
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    pr = _dev_ptr(rho, (nzm, ncrms), "rho", f.dtype)
    pa = _dev_ptr(adz, (nzm, ncrms), "adz", f.dtype)
    ntr = 0 if cpath is None or cpath.dim() != 3 else int(cpath.shape[0])
    sh = column_cond_shapes(n, nxp6 - 6, nzm + 1, ntr)
    P = {k: None if t is None else _dev_ptr(t, sh[k], k, f.dtype)
         for k, t in (("lo", lo), ("hi", hi), ("kcnt", kcnt), ("kbot", kbot), ("ktop", ktop), ("cpath", cpath), ("cover", cover),
                      ("mass", mass))}
    fn = lib().mpdata_column_cond_device if f.dtype == torch.float64 else lib().mpdata_column_cond_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, pr, pa, int(tc), P["lo"], P["hi"], P["kcnt"], P["kbot"], P["ktop"],
              P["cpath"], P["cover"], P["mass"], int(first_tracer), ntr, _stream_handle(stream)))


def vsolve_shapes(n, nz):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a vsolve call on n instances: lo, di, up
    (nzm, n)."""
    n, nz = int(n), int(nz)
    return {"lo": (nz - 1, n), "di": (nz - 1, n), "up": (nz - 1, n)}


def vsolve(f, lo, di, up, sl0=0, n=None, stream=None):
    """Implicit vertical solve (include/mpdata_hip.h 3o) of instances [sl0, sl0+n) (default: the rest from sl0) of a
    reference-layout DEVICE tensor f ([ntr,] nzm, nx+6, ncrms), float64 or float32, in place; lo, di, up of the same dtype
    with the shapes of vsolve_shapes(n, nz).  Enqueued on `stream`; returns when the work is done (mpdata_vsolve_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"vsolve: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() not in (3, 4) or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f")
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    sh = vsolve_shapes(n, nzm + 1)
    ptrs = [None if t is None else _dev_ptr(t, sh[k], k, f.dtype) for k, t in (("lo", lo), ("di", di), ("up", up))]
    fn = lib().mpdata_vsolve_device if f.dtype == torch.float64 else lib().mpdata_vsolve_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, *ptrs, _stream_handle(stream)))


def vdiffuse_shapes(n, nx, nz):
    """Torch shapes (reversed-axes view of the reference layout) of the arrays of a vdiffuse call on n instances: tkh (nzm,
    nx+2, n), cz (nzm, n), sb, st (nx, n)."""
    n, nx, nz = int(n), int(nx), int(nz)
    return {"tkh": (nz - 1, nx + 2, n), "cz": (nz - 1, n), "sb": (nx, n), "st": (nx, n)}


def vdiffuse(f, rho, adz, tkh, cz, sb=None, st=None, sl0=0, n=None, stream=None):
    """Implicit vertical diffusion with a per-cell diffusivity (include/mpdata_hip.h 3s) of instances [sl0, sl0+n) (default:
    the rest from sl0) of a reference-layout DEVICE tensor f ([ntr,] nzm, nx+6, ncrms) with rho, adz (nzm, ncrms), float64 or
    float32, in place; tkh, cz, sb, st of the same dtype with the shapes of vdiffuse_shapes(n, nx, nz) (sb, st may be None).
    Enqueued on `stream`; returns when the work is done (mpdata_vdiffuse_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"vdiffuse: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() not in (3, 4) or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f")
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    n = ncrms - int(sl0) if n is None else int(n)
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    pr = _dev_ptr(rho, (nzm, ncrms), "rho", f.dtype)
    pa = _dev_ptr(adz, (nzm, ncrms), "adz", f.dtype)
    sh = vdiffuse_shapes(n, nxp6 - 6, nzm + 1)
    ptrs = [None if t is None else _dev_ptr(t, sh[k], k, f.dtype) for k, t in (("tkh", tkh), ("cz", cz), ("sb", sb), ("st", st))]
    fn = lib().mpdata_vdiffuse_device if f.dtype == torch.float64 else lib().mpdata_vdiffuse_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, int(sl0), n, pf, pr, pa, *ptrs, _stream_handle(stream)))


def subside_device(f, cb, cc, dsum=None, stream=None):
    """Large-scale vertical advection (include/mpdata_hip.h 3m) on every column of a reference-layout DEVICE tensor f
    ([ntr,] nzm, nx+6, ncrms), float64 or float32, in place; cb, cc (nzm, ncrms) and dsum ([ntr,] nzm, ncrms) or None of the
    same dtype.  Enqueued on `stream`; returns when the work is done (mpdata_subside_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"subside_device: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() not in (3, 4) or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f")
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    pb = _dev_ptr(cb, (nzm, ncrms), "cb", f.dtype)
    pc = _dev_ptr(cc, (nzm, ncrms), "cc", f.dtype)
    pd = None if dsum is None else _dev_ptr(dsum, tuple(f.shape[:-3]) + (nzm, ncrms), "dsum", f.dtype)
    fn = lib().mpdata_subside_device if f.dtype == torch.float64 else lib().mpdata_subside_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, pf, pb, pc, pd, _stream_handle(stream)))


def level_add(f, d, mode=LEVEL_ADD, stream=None):
    """f(sl, i, k, t) += d(sl, k, t) on every column of a reference-layout DEVICE tensor f ([ntr,] nzm, nx+6, ncrms), float64
    or float32, in place; d ([ntr,] nzm, ncrms) of the same dtype; mode LEVEL_ADD_CLIP: max(0, .) of the sum.  Asynchronous
    on `stream` (mpdata_level_add_device)."""
    import torch
    if f.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"level_add: dtype {f.dtype} is neither float64 nor float32")
    if f.dim() not in (3, 4) or f.shape[-2] < 7:
        raise MpdataError(-1, f"f: shape {tuple(f.shape)} is no reference-layout f")
    nt = f.shape[0] if f.dim() == 4 else 1
    nzm, nxp6, ncrms = f.shape[-3:]
    pf = _dev_ptr(f, tuple(f.shape), "f", f.dtype)
    pd = _dev_ptr(d, tuple(f.shape[:-3]) + (nzm, ncrms), "d", f.dtype)
    fn = lib().mpdata_level_add_device if f.dtype == torch.float64 else lib().mpdata_level_add_f32_device
    _check(fn(ncrms, nxp6 - 6, nzm + 1, nt, pf, pd, int(mode), _stream_handle(stream)))


def scale_uw(u, w, su=None, sw=None, stream=None):
    """u(sl, :, :) *= su(sl), w(sl, :, :) *= sw(sl) on reference-layout DEVICE tensors u (nzm, nx+5, ncrms), w (nz, nx+4,
    ncrms), float64 or float32, in place -- every column and level, level nz of w included; su, sw (ncrms,) of the same
    dtype.  u or w may be None together with its factor.  Asynchronous on `stream` (mpdata_scale_uw_device)."""
    import torch
    a = u if u is not None else w
    if a is None:
        raise MpdataError(-1, "scale_uw: u and w are both None")
    if a.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"scale_uw: dtype {a.dtype} is neither float64 nor float32")
    if a.dim() != 3 or (u is not None and w is not None and w.dim() != 3):
        raise MpdataError(-1, f"scale_uw: shape {tuple(a.shape)} is no reference-layout u or w")
    ncrms = a.shape[-1]
    nx = u.shape[1] - 5 if u is not None else w.shape[1] - 4
    nz = u.shape[0] + 1 if u is not None else w.shape[0]
    ptrs = [None if t is None else _dev_ptr(t, sh, k, a.dtype)
            for k, t, sh in (("u", u, (nz - 1, nx + 5, ncrms)), ("w", w, (nz, nx + 4, ncrms)), ("su", su, (ncrms,)), ("sw", sw, (ncrms,)))]
    fn = lib().mpdata_scale_uw_device if a.dtype == torch.float64 else lib().mpdata_scale_uw_f32_device
    _check(fn(ncrms, nx, nz, *ptrs, _stream_handle(stream)))


def courant(u, w, rho, adz, clev=None, cinst=None, stream=None):
    """Outflow Courant number (include/mpdata_hip.h 3h) of reference-layout DEVICE tensors u (nzm, nx+5, ncrms), w (nz,
    nx+4, ncrms), rho, adz (nzm, ncrms), float64 or float32, into device tensors clev (nzm, ncrms) and / or cinst (ncrms,)
    of the same dtype (None = not wanted), asynchronous on `stream` (mpdata_courant_device)."""
    import torch
    if u.dtype not in (torch.float64, torch.float32):
        raise MpdataError(-1, f"courant: dtype {u.dtype} is neither float64 nor float32")
    if u.dim() != 3 or u.shape[1] < 6:
        raise MpdataError(-1, f"u: shape {tuple(u.shape)} is no reference-layout u")
    nzm, nxp5, ncrms = u.shape
    sh = shapes(ncrms, nxp5 - 5, nzm + 1, 1)
    ptrs = [_dev_ptr(t, sh[k], k, u.dtype) for k, t in (("u", u), ("w", w), ("rho", rho), ("adz", adz))]
    if clev is None and cinst is None:
        raise MpdataError(-1, "courant: clev and cinst are both None")
    pl = None if clev is None else _dev_ptr(clev, (nzm, ncrms), "clev", u.dtype)
    pi = None if cinst is None else _dev_ptr(cinst, (ncrms,), "cinst", u.dtype)
    fn = lib().mpdata_courant_device if u.dtype == torch.float64 else lib().mpdata_courant_f32_device
    _check(fn(ncrms, nxp5 - 5, nzm + 1, *ptrs, pl, pi, _stream_handle(stream)))


def fill_synthetic(t, name, seed, dist, ncrms_global=None, sl0=0, stream=None):
    """Fill device tensor `t` (reversed-axes layout, last axis = local CRM
    instances) with the synthetic law of array `name`."""
    nloc = t.shape[-1]
    rows = t.numel() // nloc
    import torch
    ng = nloc if ncrms_global is None else ncrms_global
    fn = lib().mpdata_fill_synthetic_device if t.dtype == torch.float64 else lib().mpdata_fill_synthetic_f32_device
    if t.dtype not in (torch.float64, torch.float32) or not t.is_contiguous():
        raise MpdataError(-1, f"{name}: need a contiguous float64 or float32 device tensor")
    _check(fn(ctypes.c_void_p(t.data_ptr()), SID[name], rows, ng, sl0, nloc, seed, dist,
              _stream_handle(stream)))


def _shard_check(t, name):
    import torch
    if not (t.is_cuda and t.is_contiguous() and t.dtype in (torch.float64, torch.float32)):
        raise MpdataError(-1, f"{name}: need a contiguous float64 or float32 device tensor")


def _shard_dims(full, shard):
    """rows, ncrms, nloc IN UNITS OF 8 BYTES for the fp64 pack kernel: an fp32 tensor is moved as
    pairs of elements, which needs even ncrms, nloc and sl0."""
    _shard_check(full, "full")
    _shard_check(shard, "shard")
    if full.dtype != shard.dtype or tuple(full.shape[:-1]) != tuple(shard.shape[:-1]):
        raise MpdataError(-1, f"shard {tuple(shard.shape)} {shard.dtype} does not match full "
                              f"{tuple(full.shape)} {full.dtype}")
    return full.numel() // full.shape[-1], full.shape[-1], shard.shape[-1]


def pack_shard(full, sl0, nloc, out=None, stream=None):
    """Contiguous copy of CRM instances [sl0, sl0+nloc) of a device tensor (float64, or
    float32 with even ncrms, nloc, sl0)."""
    import torch
    if out is None:
        out = torch.empty(full.shape[:-1] + (nloc,), dtype=full.dtype, device=full.device)
    rows, ncrms, nl = _shard_dims(full, out)
    if nl != nloc:
        raise MpdataError(-1, f"out holds {nl} instances, asked for {nloc}")
    if full.dtype == torch.float32:
        if (ncrms | nloc | sl0) & 1:
            raise MpdataError(-1, "float32 shards need even ncrms, nloc and sl0")
        ncrms, nloc, sl0 = ncrms // 2, nloc // 2, sl0 // 2
    _check(lib().mpdata_pack_shard_device(ctypes.c_void_p(full.data_ptr()),
                                          ctypes.c_void_p(out.data_ptr()), rows, ncrms, sl0, nloc,
                                          _stream_handle(stream)))
    return out


def unpack_shard(full, shard, sl0, stream=None):
    import torch
    rows, ncrms, nloc = _shard_dims(full, shard)
    if full.dtype == torch.float32:
        if (ncrms | nloc | sl0) & 1:
            raise MpdataError(-1, "float32 shards need even ncrms, nloc and sl0")
        ncrms, nloc, sl0 = ncrms // 2, nloc // 2, sl0 // 2
    _check(lib().mpdata_unpack_shard_device(ctypes.c_void_p(full.data_ptr()),
                                            ctypes.c_void_p(shard.data_ptr()), rows, ncrms, sl0,
                                            nloc, _stream_handle(stream)))
