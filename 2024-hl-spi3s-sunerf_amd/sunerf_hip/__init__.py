"""MI355X-native kernels of the SuNeRF ray-march renderer (binding layer; see include/sunerf_hip.h)."""
from .lib import LIB_PATH, EXPORTED_SYMBOLS, EXTENSION_SYMBOLS, RESPONSE_SYMBOLS, PREP_SYMBOLS, INSTRUMENT_SYMBOLS, PATCH_SYMBOLS, LIKELIHOOD_SYMBOLS, SSIM_LOSS_SYMBOLS, DECONVOLVE_SYMBOLS, PSF_GRAD_SYMBOLS, DESPIKE_SYMBOLS, COALIGN_SYMBOLS, STACK_SYMBOLS, NOISE_GATE_SYMBOLS, REGISTER_SYMBOLS, ENHANCE_SYMBOLS, SunerfHipError, load  # noqa: F401
# (the name sunerf_hip.ssim_loss is the function from here on; `from sunerf_hip.ssim_loss import ...` still reaches the module)
from .ssim_loss import patch_ssim, ssim_loss  # noqa: F401,E402
