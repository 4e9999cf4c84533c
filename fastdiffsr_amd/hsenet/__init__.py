"""HSENet (MSI_SR_model/model/hsenet.py) inference on the HIP engine."""
from ..swinir.model import to_u8  # noqa: F401
from .arch import HSENetConfig, state_schema, tap_names  # noqa: F401
from .model import HSENet, load_synthetic  # noqa: F401
