"""MI355X replacement of the ``torch_harmonics`` surface the reference uses
(``RealSHT``, ``InverseRealSHT``, ``quadrature.legendre_gauss_weights``), plus the
per-degree ``power_spectrum`` of a coefficient tensor."""
from . import quadrature  # noqa: F401
from .sht import InverseRealSHT, RealSHT, adopt  # noqa: F401
from .spectrum import power_spectrum  # noqa: F401
