"""MI355X-native kernels of the SuNeRF ray-march renderer (binding layer; see include/sunerf_hip.h)."""
from .lib import LIB_PATH, EXPORTED_SYMBOLS, EXTENSION_SYMBOLS, RESPONSE_SYMBOLS, PREP_SYMBOLS, INSTRUMENT_SYMBOLS, PATCH_SYMBOLS, LIKELIHOOD_SYMBOLS, SunerfHipError, load  # noqa: F401
