"""
psa_amd -- MI355X-native implementation of the PSA spectral-energy-density hot path.

Switching from the reference is an import change:

    from psa import Trajectory, SED, SEDCalculator          # h-walk/PSA (NumPy, CPU)
    from psa_amd import Trajectory, SED, SEDCalculator      # this package (HIP, gfx950)

Only what the SED path needs is here: the three core classes,
`parse_direction`, the ctypes binding of libpsa_hip.so, k-point sharding over RCCL and the
synthetic-trajectory generator used by the benchmark.  Loaders, plotting, CLI and GUI of the
reference are out of scope.
"""
from .core import SED, SEDCalculator, Trajectory
from .core.sed import fast_intensity
from .utils.helpers import parse_direction
from .segments import Segments
from .modes import ModeSED, site_groups
from .covariance import ModeVectors, mode_vectors, spectral_weights
from .peaks import PeakFit, fit_peaks
from .vdos import VDOS
from .dynamic import DynamicSpectra
from .lattice import PowderSpectra, commensurate_vectors, shell_bins
from .partial import PartialSpectra, PowderPartialSpectra
from .self_spectra import draw_atoms
from .correlations import PowderTimeCorrelations, TimeCorrelations, relaxation_time
from .displacements import MeanSquareDisplacement, VanHoveSelf
from .overlap import DynamicOverlap
from .pairs import RadialDistribution, VanHoveDistinct, max_pair_radius
from .angles import BondAngleDistribution
from .order import BondOrder
from .clusters import SolidClusters
from .persistence import BondPersistence
from .cna import CommonNeighbours
from .acna import AdaptiveCommonNeighbours
from .local_order import LocalOrder, wigner_3j_table
from .weights import mass_weights

__version__ = "0.2.0"
__all__ = ["Trajectory", "SED", "SEDCalculator", "parse_direction", "fast_intensity", "mass_weights", "Segments",
           "VDOS", "DynamicSpectra", "PowderSpectra", "PartialSpectra", "PowderPartialSpectra", "commensurate_vectors", "shell_bins", "draw_atoms", "TimeCorrelations", "PowderTimeCorrelations", "relaxation_time", "MeanSquareDisplacement", "VanHoveSelf", "DynamicOverlap", "RadialDistribution", "VanHoveDistinct", "max_pair_radius", "BondAngleDistribution", "BondOrder", "LocalOrder", "wigner_3j_table", "SolidClusters", "BondPersistence", "CommonNeighbours", "AdaptiveCommonNeighbours", "ModeSED", "site_groups", "PeakFit", "fit_peaks", "ModeVectors",
           "mode_vectors", "spectral_weights", "__version__"]
