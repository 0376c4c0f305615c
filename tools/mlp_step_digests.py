"""SHA-256 digests of what the fused PPO MLP optimizer step computes on seeded inputs (tests/mlp_digest_cases.py), as JSON on
stdout: gradients, acc, advantage moments, parameters and Adam moments after two steps at four shapes.  Needs an MI355X.

    python tools/mlp_step_digests.py > tests/golden/mlp_step_digests.json

Run on the build a change of the kernels has to reproduce bit for bit (the parent commit's), commit the output, and
tests/test_ppo_mlp_resident.py::test_same_bits_as_the_recorded_build holds every later build to it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402,F401  (before the library: it binds to the HIP runtime torch has loaded)

from myochallenge_amd import native  # noqa: E402
import mlp_digest_cases  # noqa: E402

if __name__ == "__main__":
    lib = native.load()
    print(json.dumps({"library": lib.version, "digests": mlp_digest_cases.step_digests(lib)}, indent=1, sort_keys=True))
