"""lanczosplusplus_amd -- MI355X-native Lanczos inner engine behind LanczosPlusPlus's
Model / Basis / InternalProductStored plug-in surface (one hot path).

The compute path is liblpp_engine.so (hand-written HIP for gfx950 + a C ABI, csrc/);
this package is the thin host layer: ctypes binding, geometry/input helpers, the
torch.distributed communicator used by the multi-GPU path.
"""
from ._capi import LIB_PATH, LppError  # noqa: F401
from .engine import (LanczosEngine, continued_fraction, new_parts, operator_plan, operator_plan_heis, operator_plan_heis_spin, operator_plan_tj, operator_string_plan, operator_string_plan_heis, operator_string_plan_tj, operator_sum_plan, partition_rows, rdm_plan, split_csr,  # noqa: F401
                     tridiag_lowest)
from . import geometry  # noqa: F401

__all__ = ["LanczosEngine", "LppError", "partition_rows", "split_csr", "tridiag_lowest", "continued_fraction", "new_parts", "operator_plan", "operator_plan_tj", "operator_plan_heis", "operator_plan_heis_spin", "operator_string_plan", "operator_string_plan_heis", "operator_string_plan_tj", "operator_sum_plan", "rdm_plan", "geometry", "LIB_PATH"]
