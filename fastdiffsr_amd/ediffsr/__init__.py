"""EDiffSR on the HIP engine: the ConditionalNAFNet noise predictor and the IR-SDE reverse process (sampling, and training through DenoisingModel)."""
from .arch import NAFNetConfig, param_schema          # noqa: F401
from .model import ConditionalNAFNet                 # noqa: F401
from .sde import IRSDE                               # noqa: F401
from .denoising_model import DenoisingModel       # noqa: F401
