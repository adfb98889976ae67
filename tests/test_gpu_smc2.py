"""-m gpu: SMC2 over ``FleetEngine`` (two fleets; cssm_fleet_copy_series clones and adopts on the device) against SMC2 over the
``OracleEngine`` of tests/test_smc2_host.py (CPU oracle handles; clones and adoptions through the host): the parameter level is the same
numpy code, so after EVERY observation theta, logw, log_evidence, ess, resampled and accepted agree bit for bit -- which holds only if
every cloned and every adopted series continues with the bits of its source.  Then the truth configuration of the host file on the GPU:
the same seeds, the same criteria, and (the same bits) the same statistics.
"""
import numpy as np
import pytest

import cases
import test_smc2_host as host
from composablestatespacemodels_amd import SMC2, FleetEngine, TimedObservation

pytestmark = pytest.mark.gpu


def both(unparam, model, draws, n, obs, **kw):
    out = []
    for engine in (FleetEngine(model, n, len(draws)), host.OracleEngine(model, n, len(draws))):
        with SMC2(unparam, draws, n, engine=engine, **kw) as smc:
            out.append((smc.run(obs), smc.rejuvenations))
    return out


def assert_agree(gpu, cpu):
    (a, ra), (b, rb) = gpu, cpu
    assert ra == rb and len(a) == len(b)
    for s, (x, y) in enumerate(zip(a, b)):
        assert x.t == y.t and x.resampled == y.resampled and x.accepted == y.accepted, (s, x, y)
        np.testing.assert_array_equal(x.theta, y.theta, err_msg=f"theta after observation {s}")
        np.testing.assert_array_equal(x.logw, y.logw, err_msg=f"logw after observation {s}")
        assert x.log_evidence == y.log_evidence and x.ess == y.ess, (s, x.log_evidence, y.log_evidence, x.ess, y.ess)


@pytest.mark.parametrize("ess_fraction", [0.5, 1.01])
def test_linear_agrees_with_the_oracle_engine(ess_fraction):
    S, n, T = 32, 65, 20
    gpu, cpu = both(host.unparam(), cases.linear_model(), host.prior_draws(S, 11), n, host.observations(T), log_prior=host.log_prior,
                    free=host.FREE, ess_fraction=ess_fraction, seed=11)
    assert_agree(gpu, cpu)
    assert gpu[1] >= 1 and sum(s.accepted for s in gpu[0]) > 0          # clones and adoptions did happen


def c2_draws(S, seed):
    rng = np.random.default_rng(seed)
    base = np.asarray(cases.c2_params().flattenParams())
    return [cases.c2_params().withFlat(base + 0.5 * rng.standard_normal(base.size)) for _ in range(S)]   # (wide enough that ESS < S / 2 once)


@pytest.mark.parametrize("ess_fraction", [0.5, 1.01])
def test_c2_agrees_with_the_oracle_engine(ess_fraction):
    S, n, T = 16, 100, 12
    t, y, has = cases.poisson_counts(T, missing=0.2)
    obs = [TimedObservation(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)]
    assert any(o.observation is None for o in obs)
    gpu, cpu = both(cases.c2_unparam(), cases.c2_model(), c2_draws(S, 5), n, obs, ess_fraction=ess_fraction, moves=2, scale=0.3, seed=5)
    assert_agree(gpu, cpu)
    assert gpu[1] == (T if ess_fraction > 1.0 else 1) and sum(s.accepted for s in gpu[0]) > 0


def test_the_truth_configuration_on_the_gpu():
    runs = []
    for r in range(host.R):
        st, n_rej = host.truth_run(lambda: FleetEngine(cases.linear_model(), host.N, host.S), host.SEED0 + r)
        runs.append(st)
        assert n_rej >= 1
    runs = np.array(runs)
    host.check_truth(runs, "smc2 / fleets")
    cpu0, _ = host.truth_run(lambda: host.OracleEngine(cases.linear_model(), host.N, host.S), host.SEED0)
    np.testing.assert_array_equal(runs[0], cpu0)                          # the same bits as the CPU run of the first seed
