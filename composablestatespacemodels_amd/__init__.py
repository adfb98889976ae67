"""composablestatespacemodels_amd -- MI355X-native bootstrap particle filter behind the
ParticleFilter / Resample / BootstrapFilter seams of jonnylaw/ComposableStateSpaceModels.

The compute path is libcssm_pf.so (hand-written HIP for gfx950, C ABI in include/cssm_pf.h).
This package is the thin host-side mirror of the reference's interface for that path.
"""
from . import _abi
from ._abi import CssmError, load_library
from .filter import FilterFleet, FilterInitFleet, FilterLgcpFleet, ForecastOut, NativeLgcpFleet, NativePfFleet, ObservationWithState, ParticleFilter
from .simulate import LgcpSim, SimulateData, SimulatedPoint, lgcp_events_data, lgcp_fleet_data, simulate, simulate_from, simulate_lgcp, simulate_lgcp_last_ms
from .streaming import Streaming
from .smc2 import SMC2, FleetEngine, Smc2State
from .if2 import IF2, IF2Single, If2Result
from .pmmh import Prior, pmmh_fleet_chains, pmmh_lgcp_fleet_chains
from .model import (Data, Model, Parameters, ParamNode, Sde, SdeParameter, TimedObservation,
                    UnparamModel, UnparamSde, logistic, logit)

__all__ = ["_abi", "CssmError", "load_library", "FilterFleet", "ForecastOut", "NativePfFleet", "NativeLgcpFleet", "FilterLgcpFleet", "FilterInitFleet", "lgcp_fleet_data", "Streaming", "SMC2", "Smc2State", "FleetEngine", "IF2", "IF2Single", "If2Result", "Prior", "pmmh_fleet_chains", "pmmh_lgcp_fleet_chains", "SimulateData", "SimulatedPoint", "simulate", "simulate_from", "LgcpSim", "simulate_lgcp", "simulate_lgcp_last_ms", "lgcp_events_data", "ObservationWithState", "ParticleFilter", "Data", "Model", "Parameters", "ParamNode", "Sde",
           "SdeParameter", "TimedObservation", "UnparamModel", "UnparamSde", "logistic", "logit"]
