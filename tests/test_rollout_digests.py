"""Every rollout path stores, bit for bit, what the build before the rollout collectors (rl/rollout.py) stored: seeded runs of
collect_rollouts / train / collect_rollouts (tests/rollout_digest_cases.py) against the SHA-256 digests that
tools/rollout_digests.py printed from that build (tests/golden/rollout_digests.json; it reproduced every group of every case in a
second process).  The rank-synchronised normaliser needs two processes and stays with the test_two_rank_* tests."""
import json
import os

import pytest

import rollout_digest_cases as cases


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "rollout_digests.json")) as f:
        return json.load(f)["digests"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_rollout_stores_the_recorded_bits(hip_lib, golden, name):
    got = cases.run_case(name)
    for group in ("rollout1", "after_train", "rollout2"):
        diff = sorted(k for k in set(got[group]) | set(golden[name][group]) if got[group].get(k) != golden[name][group].get(k))
        assert not diff, (name, group, diff)
