"""adafortitran_amd -- MI355X (gfx950) native AdaFortiTran / FortiTran forward path.

Package contents (only what the hot path needs):
  csrc/          hand-written HIP kernels + the C ABI (include/adafortitran_amd.h)
  _lib, _abi     ctypes binding of that ABI (fails loudly when the .so is missing)
  hip_ops        pointer tables / workspace / per-stage calls on torch device memory
  estimators     drop-in mirror of the reference's src/models module surface
  blocks         parameter containers + the autograd (training) composite
  config         YAML/pydantic config surface
  synth          deterministic synthetic weights + inputs
  metrics        channel-MSE metric (device reduction + RCCL all-gather)
  lmmse          the LMMSE (Wiener) baseline of the channel simulator, one slot or a window of slots: definition, closed-form MSE, nn.Module;
                 its design point chosen from the pilots (ConditionEstimator, EstimatedConditions)
                 and the full-grid smoother a decision-directed receiver re-estimates with (lmmse_grid_host)
  linksim        the link the estimates are measured on (bit errors, rates, coded blocks) and DataAidedRefiner, the receiver loop that
                 refines an estimate from its own decisions
"""
from .config import ModelConfig, SystemConfig, load_config  # noqa: F401
from .estimators import (AdaFortiTranEstimator, BaseFortiTranEstimator, FortiTranEstimator,  # noqa: F401
                         LinearEstimator)
from .linksim import DataAidedRefiner  # noqa: F401
from .lmmse import ConditionEstimator, EstimatedConditions, LmmseEstimator, lmmse_classify_host, lmmse_grid_host  # noqa: F401

__version__ = "0.1.0"
