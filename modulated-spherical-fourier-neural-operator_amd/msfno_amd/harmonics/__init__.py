"""MI355X replacement of the ``torch_harmonics`` surface the reference uses
(``RealSHT``, ``InverseRealSHT``, ``quadrature.legendre_gauss_weights``), plus the
per-degree ``power_spectrum`` of a coefficient tensor and the vector transforms
(``RealVectorSHT``, ``InverseRealVectorSHT``) with the wind diagnostics built on them, and
Gaussian random fields on the sphere (``GaussianRandomFieldS2``, ``SphericalAR1``)."""
from . import quadrature  # noqa: F401
from .random_fields import (GaussianRandomFieldS2, SphericalAR1,  # noqa: F401
                            field_variance, matern_sqrt_eig, unit_variance)
from .sht import InverseRealSHT, RealSHT, adopt  # noqa: F401
from .spectrum import power_spectrum  # noqa: F401
from .vector import (InverseRealVectorSHT, RealVectorSHT,  # noqa: F401
                     divergence_vorticity_spectra, uv_to_vector, vector_to_uv,
                     vorticity_divergence, wind_from_vorticity_divergence)
