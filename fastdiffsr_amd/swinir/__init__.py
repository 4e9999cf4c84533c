"""SwinIR, the transformer comparator of MSI_SR_model/, on the HIP engine: inference in exact fp32 (model.SwinIR), the test
command line (python -m fastdiffsr_amd.swinir.test)."""
from .arch import SwinIRConfig, param_schema, state_schema, tap_names  # noqa: F401
from .model import SwinIR, load_synthetic, to_u8  # noqa: F401
