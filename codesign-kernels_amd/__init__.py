"""codesign-kernels_amd -- MI355X-native E3SM-MMF 2D MPDATA tracer advection.

Host-side mirror (Python) of the one routine this project replaces:
`advect_scalar2D(f,u,w,rho,rhow,flux)` of the reference
mmf-mpdata-tracer/advect_scalar2D_pushncols_openacc.F90 (:72, :247, :477),
bound to libmpdata_hip.so (hand-written HIP for gfx950) through the C-ABI in
include/mpdata_hip.h.  The Fortran driver + shim that north_star asks for live
in fortran/; this Python face exists for bench.py, the tests and
torch.distributed plumbing.  There is no CPU fallback here: if the HIP library
is missing or no device is usable, calls raise.
"""
from .capi import (EINVAL, EUNSUPPORTED, ESTATE, ECOMM, LAYOUT_REFERENCE, LAYOUT_WAVEMAJOR, BOUNDARY_GIVEN, BOUNDARY_PERIODIC, MpdataError, Plan, VARIANT_EXACT, VARIANT_FAST, advect_scalar2D,
                   advect_scalar2D_host, release_host_buffers, algorithmic_bytes, build_library, debug_stages, device_count,
                   empty_staggered, fill_synthetic, get_variant, host_shapes, lib, lib_path, pack_shard, periodic_halo,
                   set_plan_layout, set_serpentine, set_tall_columns, set_f32_odd_ncrms, level_window, level_stats, courant, level_add, scale_uw, column_path, column_path_shapes, column_cond, column_cond_shapes, diffuse, diffuse_shapes, subside_device, sediment, sediment_shapes, vsolve, vsolve_shapes, cell_add, cell_add_shapes, column_step_device, column_step_shapes, relax, relax_shapes, nonneg, nonneg_shapes, vdiffuse, vdiffuse_shapes, convert, convert_shapes, CONVERT_LIMIT, combine, combine_shapes, COMBINE_CLIP, COMBINE_MAX, column_scan, column_scan_shapes, COLUMN_SCAN_DOWN, COLUMN_SCAN_EXCLUSIVE, level_hist, level_hist_shapes, LEVEL_HIST_MAX_BINS, level_draft, level_draft_shapes, satadj, satadj_shapes, SatadjParams, SATADJ_ICE, level_cov, level_cov_shapes, LEVEL_COV_RAW, level_cond, level_cond_shapes, CELL_ADD, CELL_ADD_CLIP, LEVEL_ADD, LEVEL_ADD_CLIP, set_tile, set_variant, set_wm_flags, version, WMF_NOSTREAM, WMF_TPW1, WMF_NOSPLIT, WMF_SPLIT, shard_range, shapes, stage_shapes, stream_ceiling, unpack_shard)
from .shard import gather_outputs, partition, scatter_inputs

__all__ = ["level_draft", "level_draft_shapes", "level_hist", "level_hist_shapes", "LEVEL_HIST_MAX_BINS", "column_scan", "column_scan_shapes", "COLUMN_SCAN_DOWN", "COLUMN_SCAN_EXCLUSIVE", "combine", "combine_shapes", "COMBINE_CLIP", "COMBINE_MAX", "satadj", "satadj_shapes", "SatadjParams", "SATADJ_ICE", "nonneg", "nonneg_shapes", "column_cond", "column_cond_shapes", "level_cond", "level_cond_shapes", "level_cov", "level_cov_shapes", "LEVEL_COV_RAW", "convert", "convert_shapes", "CONVERT_LIMIT", "vdiffuse", "vdiffuse_shapes", "relax", "relax_shapes", "column_step_device", "column_step_shapes", "cell_add", "cell_add_shapes", "CELL_ADD", "CELL_ADD_CLIP", "vsolve", "vsolve_shapes", "sediment", "sediment_shapes", "subside_device", "diffuse", "diffuse_shapes", "column_path", "column_path_shapes", "scale_uw", "level_add", "LEVEL_ADD", "LEVEL_ADD_CLIP", "courant", "level_stats", "set_tall_columns", "set_f32_odd_ncrms", "level_window", "EINVAL", "EUNSUPPORTED", "ESTATE", "ECOMM", "set_serpentine", "set_wm_flags", "version", "WMF_NOSTREAM", "WMF_TPW1", "WMF_NOSPLIT", "WMF_SPLIT", "LAYOUT_REFERENCE", "LAYOUT_WAVEMAJOR", "BOUNDARY_GIVEN", "BOUNDARY_PERIODIC", "periodic_halo", "host_shapes", "set_plan_layout", "shard_range", "stream_ceiling", "MpdataError", "Plan", "VARIANT_EXACT", "VARIANT_FAST", "advect_scalar2D",
           "advect_scalar2D_host", "release_host_buffers", "algorithmic_bytes", "build_library", "debug_stages", "device_count",
           "empty_staggered", "fill_synthetic", "get_variant", "lib", "lib_path", "pack_shard", "set_tile",
           "set_variant", "shapes", "stage_shapes", "unpack_shard", "partition", "scatter_inputs",
           "gather_outputs"]
