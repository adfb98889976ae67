// cssm::Filter::filterForecasts / filterForecastsMore / stepForecast (include/cssm_pf.hpp) against the C ABI they wrap.  Compiled and
// linked by tests/test_filter_forecasts_host.py (the signatures); run with a particle count by tests/test_gpu_filter_forecasts.py:
// it prints, per route, the obs_mean / eta_lower / state_upper[0] of every row as hex doubles.
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "cssm_pf.hpp"

using namespace cssm;

static_assert(std::is_same<decltype(&Filter::filterForecasts),
                           std::pair<double, std::vector<ForecastOut>> (Filter::*)(const std::vector<Data>&, double)>::value,
              "filterForecasts(data, interval) -> (ll, [ForecastOut] x T)");
static_assert(std::is_same<decltype(&Filter::filterForecastsMore),
                           std::pair<double, std::vector<ForecastOut>> (Filter::*)(const std::vector<Data>&, double)>::value,
              "filterForecastsMore(data, interval) -> (ll, [ForecastOut] x T)");
static_assert(std::is_same<decltype(&Filter::stepForecast), std::pair<PfState, ForecastOut> (Filter::*)(const PfState&, const Data&, double)>::value,
              "stepForecast(s, y, interval) -> (PfState, ForecastOut)");

static void print(const char* route, double ll, const std::vector<ForecastOut>& outs) {
  std::printf("%s ll %a rows %zu\n", route, ll, outs.size());
  for (const ForecastOut& f : outs) std::printf("%s row %a %a %a %a\n", route, f.t, f.obs, f.etaIntervals.lower, f.stateIntervals[0].upper);
}

int main(int argc, char** argv) {
  const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1000;
  // C2 of tests/cpp/test_hpp.cpp: Model.poisson(Sde.ouProcess(1)) |+| Model.seasonal(24, 1, Sde.ouProcess(2)), and its eight records
  UnparamModel um = Model::poisson(Sde::ouProcess(1)) | Model::seasonal(24, 1, Sde::ouProcess(2));
  Parameters p = Parameters{{std::nullopt, SdeParameter::ouParameter({0.0}, {1.0}, {0.2}, {0.0}, {0.3})}} |
                 Parameters{{std::nullopt, SdeParameter::ouParameter({0.0}, {1.0}, {0.2}, {1.0}, {0.3})}};
  ParamModel mod(um, p);
  std::vector<Data> data;
  const double ys[] = {2, 1, 4, 0, 3, 2, 5, 1};
  for (int i = 0; i < 8; ++i) data.push_back({(double)i, i == 3 ? std::optional<double>{} : std::optional<double>{ys[i]}});
  try {
    Filter f(mod, n);
    auto r = f.filterForecasts(data, 0.9);
    print("batch", r.first, r.second);
  } catch (const std::exception& e) {
    std::printf("exception %s\n", e.what());
    return 1;
  }
  {
    Filter f(mod, n);
    std::vector<Data> a(data.begin(), data.begin() + 3), b(data.begin() + 3, data.end());
    auto r0 = f.filterForecasts(a, 0.9);
    auto r1 = f.filterForecastsMore(b, 0.9);
    r0.second.insert(r0.second.end(), r1.second.begin(), r1.second.end());
    print("more", r1.first, r0.second);
  }
  {
    Filter f(mod, n);
    PfState s = f.initialiseState(0.0);
    std::vector<ForecastOut> outs;
    for (const Data& y : data) { auto r = f.stepForecast(s, y, 0.9); s = r.first; outs.push_back(r.second); }
    print("stream", s.ll, outs);
  }
  return 0;
}
