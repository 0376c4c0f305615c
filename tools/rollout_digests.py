"""SHA-256 digests of what seeded PPO runs store on every rollout path (tests/rollout_digest_cases.py), as JSON on stdout: the six
rollout buffers, the carried-over policy input and LSTM state, the normaliser and the episode log after two rollouts, and the
parameters after the update between them.  Needs an MI355X.

    python tools/rollout_digests.py > tests/golden/rollout_digests.json

Run on the build a change of the rollout's host wiring has to reproduce bit for bit (the parent commit's), twice in two processes
to see that the build reproduces itself, commit the output, and tests/test_rollout_digests.py holds every later build to it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402,F401  (before the library: it binds to the HIP runtime torch has loaded)

from myochallenge_amd import native  # noqa: E402
import rollout_digest_cases  # noqa: E402

if __name__ == "__main__":
    lib = native.load()
    print(json.dumps({"library": lib.version, "build_id": lib.build_id, "digests": rollout_digest_cases.rollout_digests(sys.argv[1:])},
                     indent=1, sort_keys=True))
