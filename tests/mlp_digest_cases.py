"""Seeded runs of the fused PPO MLP optimizer step (myo_ppo_mlp_step + myo_adam_step through FusedPPOStep.run_indexed, the
stateless path) whose outputs are reduced to SHA-256 digests: what tools/mlp_step_digests.py prints and
tests/test_ppo_mlp_resident.py compares with tests/golden/mlp_step_digests.json.  The golden file was printed by that tool on an
MI355X with the library built from the commit BEFORE the resident-image step (same inputs, same torch): a build whose kernels
keep every floating-point sum's operands and order reproduces it bit for bit.

Inputs: test_ppo_mlp_kernels.step_case (rollout arrays larger than the minibatch, shuffled index list) at the four shapes below —
OP = 32 / 64 / 128, one to three head tiles, two and four k-steps per weight-gradient split."""
import hashlib

import torch

# (O, A, B, advantage offset)
CASES = [(1, 1, 1024, 0.0), (33, 17, 1024, 0.0), (97, 48, 1024, 0.0), (86, 39, 2048, 0.0)]
CLIP, VF_COEF, ENT_COEF, LR, MAX_NORM = 0.2, 0.7, 0.01, 3e-4, 0.5
case_id = lambda c: "O%d-A%d-B%d" % c[:3]


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def make_run(lib, case, hp_limit=0.0):
    """(policy, FlatAdam, FusedPPOStep, hyper-parameter block, device inputs) of a case, wired as rl/ppo.py wires one rank."""
    from test_ppo_mlp_kernels import build_policy, step_case
    from myochallenge_amd import native
    from myochallenge_amd.rl.fused_mlp import FlatAdam, FusedPPOStep, flatten_parameters
    dev = torch.device("cuda:0")
    O, A, B, off = case
    c = step_case(O, A, B, off)
    pol = build_policy(O, A, c["seed"]).to(dev)
    fa = FlatAdam(flatten_parameters(pol), lib, LR, MAX_NORM)
    step = FusedPPOStep(pol, lib, CLIP, ENT_COEF, VF_COEF)
    fa.shadow, step.adam_syncs_shadow, step.adam = step.half[0], True, fa
    step.refresh_shadow()
    hp = torch.zeros(native.HP_WORDS, device=dev)
    hp[:3] = torch.tensor([LR, CLIP, hp_limit], device=dev)
    fa.hp = step.hp = hp
    data = [c[k].to(dev) for k in ("obs", "act", "oldlp", "adv", "ret", "idx")]
    return pol, fa, step, hp, data


def step_digests(lib, steps=2):
    """{case: {"step<k>.<what>": sha256}}: gradient vector, acc, advantage moments after each minibatch step, and parameters and
    Adam moments after the optimizer step that follows it."""
    out = {}
    for case in CASES:
        pol, fa, step, hp, data = make_run(lib, case)
        d = {}
        for k in range(steps):
            step.run_indexed(*data)
            torch.cuda.synchronize()
            assert fa.presummed > 0, "the step fell back to the GEMM path"
            d["step%d.grads" % k], d["step%d.acc" % k], d["step%d.stats" % k] = sha(fa.flat["g"]), sha(step.acc), sha(step.stats)
            fa.step()
            torch.cuda.synchronize()
            d["step%d.p" % k], d["step%d.m" % k], d["step%d.v" % k] = sha(fa.flat["p"]), sha(fa.m), sha(fa.v)
        out[case_id(case)] = d
    return out
