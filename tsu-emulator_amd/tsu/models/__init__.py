"""Energy-based models (reference: tsu/models/__init__.py:11-13) plus the README's IsingModel2D facade."""
from .ising import (IsingChain, IsingConfig, IsingGrid, IsingModel, IsingModel2D, IsingModel3D, LatticeTempering, LatticeTempering3D, PopulationAnnealing,
                    PopulationAnnealing3D, population_annealing_scan, population_annealing_scan_3d,
                    demonstrate_phase_transition, temperature_scan, temperature_scan_3d, tempering_scan, tempering_scan_3d,
                    cluster_estimators, LatticeTemperingEnsemble, LatticeTemperingEnsemble3D, edwards_anderson_samples, ensemble_summary,
                    tempering_ensemble_scan, tempering_ensemble_scan_3d, MultispinGlass3D, multispin_scan_3d,
                    multispin_quench_3d, MultispinTempering3D, multispin_tempering_scan_3d)
from .graph_tempering import GraphTempering
from .potts import PottsModel2D, PottsModel3D, potts_temperature_scan, potts_temperature_scan_3d
from .potts_muca import PottsMulticanonical, potts_multicanonical_scan
from .potts_tempering import PottsTempering, PottsTempering3D, potts_tempering_scan, potts_tempering_scan_3d
from .potts_population import (PottsPopulationAnnealing, PottsPopulationAnnealing3D, potts_population_annealing_scan,
                               potts_population_annealing_scan_3d)

__all__ = ["IsingModel", "IsingChain", "IsingGrid", "IsingModel2D", "IsingConfig", "demonstrate_phase_transition", "temperature_scan", "cluster_estimators",
           "LatticeTempering", "tempering_scan", "IsingModel3D", "temperature_scan_3d", "LatticeTempering3D", "tempering_scan_3d",
           "PopulationAnnealing", "PopulationAnnealing3D", "population_annealing_scan", "population_annealing_scan_3d",
           "LatticeTemperingEnsemble", "LatticeTemperingEnsemble3D", "edwards_anderson_samples", "ensemble_summary",
           "tempering_ensemble_scan", "tempering_ensemble_scan_3d", "MultispinGlass3D", "multispin_scan_3d", "GraphTempering",
           "PottsModel2D", "potts_temperature_scan", "PottsModel3D", "potts_temperature_scan_3d",
           "PottsMulticanonical", "potts_multicanonical_scan",
           "PottsTempering", "PottsTempering3D", "potts_tempering_scan", "potts_tempering_scan_3d",
           "PottsPopulationAnnealing", "PottsPopulationAnnealing3D", "potts_population_annealing_scan", "potts_population_annealing_scan_3d",
           "multispin_quench_3d", "MultispinTempering3D", "multispin_tempering_scan_3d"]
