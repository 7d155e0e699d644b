from . import density  # noqa: F401
from . import nufft  # noqa: F401
