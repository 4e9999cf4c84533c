"""HAT, the hybrid-attention comparator of MSI_SR_model/, on the HIP engine: inference in exact fp32 (model.HAT), the test
command line (python -m fastdiffsr_amd.hat.test)."""
from .arch import HATConfig, param_schema, state_schema, tap_names  # noqa: F401
from .model import HAT, load_synthetic, to_u8  # noqa: F401
