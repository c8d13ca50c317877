"""MI355X-native kernels of the SuNeRF ray-march renderer (binding layer; see include/sunerf_hip.h)."""
from .lib import LIB_PATH, TABLES, symbols, SunerfHipError, load  # noqa: F401
# (the name sunerf_hip.ssim_loss is the function from here on; `from sunerf_hip.ssim_loss import ...` still reaches the module)
from .ssim_loss import patch_ssim, ssim_loss  # noqa: F401,E402
