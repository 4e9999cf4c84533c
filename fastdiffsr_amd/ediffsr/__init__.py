"""EDiffSR on the HIP engine: the ConditionalNAFNet noise predictor and the IR-SDE reverse process (sampling only)."""
from .arch import NAFNetConfig, param_schema          # noqa: F401
from .model import ConditionalNAFNet                 # noqa: F401
from .sde import IRSDE                               # noqa: F401
