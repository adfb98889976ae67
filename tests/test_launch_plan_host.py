"""CPU-only check of the launch plan (csrc/cssm_launch_plan.cpp): the handle's geometry, the plan of a propagate launch and the plan of
the resampling launch behind it are pure functions of a few integers, so a table of configurations runs through them as a stand-alone
program with its own main (tests/cpp/launch_plan_main.cpp), built with -fsanitize=address,undefined and run here: host code, no device,
nothing preloaded.  The program holds every plan of its table, and of a denser sweep around it, to what must be true of any plan; this
file compares every plan of the table with the pinned tests/golden/launch_plans.json.

The pinned table is a record of the decisions as they stood when they were moved out of cssm_pf.hip, not an independent truth: a change
of a threshold changes it on purpose.  `python tests/test_launch_plan_host.py --record` writes it again."""
from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.json")
KEY_FIELDS = "n, d and what differs from a default handle's first launch (systematic, Poisson, every option at its default, wparity 1)"
VALUE_FIELDS = "stride ntiles sup nunits split nsums | do_sums geo chunk grid one slot_set want_grp grp_layout want_ws shard_slim reduce " \
               "reduce_grid reduce_per_unit | tile_sums lean_layout tile_sums_flags split s2_par offspring_kernel | the redone observation: " \
               "chunk grid one | its resampling, as before"


def plans(workdir):
    csrc = os.path.join(ROOT, "composablestatespacemodels_amd", "csrc")
    exe = os.path.join(str(workdir), "launch_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "launch_plan_main.cpp"), os.path.join(csrc, "cssm_launch_plan.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "launch_plan: ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        if " => " in line:
            key, value = line.split(" => ")
            assert key not in out, key
            out[key] = value
    return out


def test_every_plan_holds_its_invariants_and_matches_the_pinned_table(tmp_path):
    got = plans(tmp_path)
    want = json.load(open(GOLDEN))["plans"]
    assert len(got) > 300 and set(got) == set(want)
    differ = [(k, want[k], got[k]) for k in want if want[k] != got[k]]
    assert not differ, (len(differ), KEY_FIELDS, VALUE_FIELDS, differ[:5])


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    with tempfile.TemporaryDirectory() as tmp:
        table = plans(tmp)
    about = ("The launch decisions of csrc/cssm_launch_plan.cpp over the table of tests/cpp/launch_plan_main.cpp, recorded when the decision "
             "expressions had been moved out of cssm_pf.hip and not rewritten: a pin of those decisions, not an independent truth.")
    with open(GOLDEN, "w") as fh:
        json.dump({"about": about, "key": KEY_FIELDS, "value": VALUE_FIELDS, "plans": table}, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{len(table)} plans -> {GOLDEN}")
