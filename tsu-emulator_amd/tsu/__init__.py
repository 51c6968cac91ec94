"""tsu -- MI355X-native drop-in for the stochastic spin-update hot path of tsu-emulator.

Scope: ``tsu.gibbs`` (GibbsSampler sweep), ``tsu.models.ising`` (IsingGrid /
"IsingModel2D" lattice sweep) and ``tsu.core`` (ThermalSamplingUnit Langevin step), with the reference's names,
signatures and error behaviour, executed by hand-written HIP kernels for gfx950 (``tsu/_lib/libtsu_hip.so``,
C ABI in ``include/tsu_hip.h``) through ctypes.  Of the reference's other sub-packages only the two benchmark suites that
time this path are mirrored (``tsu.benchmarks``: sampling, optimisation, runner); api, ml, visualization, demos and cli are
callers of this path and are not part of this package.
"""

__version__ = "0.1.0"

from .core import (  # noqa: F401
    ConfigurationError,
    MixtureEnergy,
    ProbabilisticNeuron,
    QuadraticEnergy,
    QuadraticForm,
    SamplingError,
    ThermalSamplingUnit,
    TSUConfig,
    TSUError,
    validate_distribution,
)
from .core import ThermalSamplingUnit as TSU  # noqa: F401
from .gibbs import GibbsConfig, GibbsSampler, HardwareEmulator  # noqa: F401
from .models import (  # noqa: F401
    GraphTempering,
    IsingChain,
    IsingGrid,
    IsingModel,
    IsingModel2D,
    IsingModel3D,
    LatticeTempering3D,
    LatticeTemperingEnsemble,
    LatticeTemperingEnsemble3D,
    MultispinGlass3D,
    MultispinTempering3D,
    PopulationAnnealing,
    PopulationAnnealing3D,
    PottsModel2D,
    PottsModel3D,
    PottsMulticanonical,
    PottsPopulationAnnealing,
    PottsPopulationAnnealing3D,
    PottsTempering,
    PottsTempering3D,
    cluster_estimators,
    demonstrate_phase_transition,
    edwards_anderson_samples,
    ensemble_summary,
    multispin_quench_3d,
    multispin_scan_3d,
    multispin_tempering_scan_3d,
    potts_multicanonical_scan,
    potts_population_annealing_scan,
    potts_population_annealing_scan_3d,
    potts_temperature_scan,
    potts_temperature_scan_3d,
    potts_tempering_scan,
    potts_tempering_scan_3d,
    temperature_scan_3d,
    tempering_ensemble_scan,
    tempering_ensemble_scan_3d,
    tempering_scan_3d,
)

__all__ = [
    "ThermalSamplingUnit", "TSU", "TSUConfig", "ProbabilisticNeuron", "validate_distribution", "TSUError",
    "ConfigurationError", "SamplingError", "QuadraticEnergy", "QuadraticForm", "MixtureEnergy",
    "GibbsSampler", "GibbsConfig", "HardwareEmulator",
    "IsingModel", "IsingChain", "IsingGrid", "IsingModel2D", "demonstrate_phase_transition",
    "IsingModel3D", "temperature_scan_3d", "LatticeTempering3D", "tempering_scan_3d", "cluster_estimators",
    "PopulationAnnealing","PopulationAnnealing3D", "PottsModel2D", "potts_temperature_scan", "PottsModel3D", "potts_temperature_scan_3d",
    "PottsMulticanonical", "potts_multicanonical_scan",
    "PottsTempering", "PottsTempering3D", "potts_tempering_scan", "potts_tempering_scan_3d",
    "PottsPopulationAnnealing", "PottsPopulationAnnealing3D", "potts_population_annealing_scan", "potts_population_annealing_scan_3d",
    "LatticeTemperingEnsemble", "LatticeTemperingEnsemble3D", "edwards_anderson_samples", "ensemble_summary",
    "tempering_ensemble_scan", "tempering_ensemble_scan_3d", "MultispinGlass3D", "multispin_scan_3d",
    "GraphTempering", "multispin_quench_3d", "MultispinTempering3D", "multispin_tempering_scan_3d",
]
