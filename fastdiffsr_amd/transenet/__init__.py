"""TransENet, the global-attention comparator of MSI_SR_model/, on the HIP engine: inference in exact fp32 (model.TransENet),
the test command line (python -m fastdiffsr_amd.transenet.test)."""
from .arch import TransENetConfig, state_schema, tap_names  # noqa: F401
from .model import TransENet, load_synthetic, to_u8  # noqa: F401
