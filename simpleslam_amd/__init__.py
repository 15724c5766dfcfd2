"""simpleslam_amd -- MI355X-native scan-to-map registration (the PCR hot path of SimpleSLAM).

Only what the path needs: csrc/ (HIP kernels + the C ABI of include/pcr_hip.h),
pcr.py (host mirror of the reference's PCR::PointCloudRegister plugin), synth.py
(deterministic synthetic clouds for tests and bench.py).
"""
from .pcr import (TIME_F32_SECONDS, TIME_F64_SECONDS, TIME_U32_NANOSECONDS, Backend, Frontend, GicpRegister, LiorfRegister, LoamRegister, NdtRegister, PcrError, PointCloudRegister, PoseGraph, ScanContext, SubMap,  # noqa: F401
                  VgicpRegister, default_params, deskew, deskew_host, global_reloc_hypotheses, global_reloc_params, kf_rank_near_host, load_library, make_register, pose_to_mobile,
                  reloc_hypotheses, reloc_params, pcd_read, pcd_write, tum_format, tum_parse)
