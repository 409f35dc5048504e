"""tests/golden/ddpg_loss_fixtures.npz: the reference's DDPG objective (warp_drive/training/algorithms/policygradient/
ddpg.py::DDPG.compute_loss_and_metrics) on seeded random batches, on the CPU -- inputs, both losses, every logged metric,
and the gradients with respect to the value and J inputs.  Run by hand with the reference on the path:

    PYTHONPATH=oracle/gym_shim:<reference checkout> python scripts/gen_ddpg_golden.py

Nothing else reads the reference: tests/test_classic_control_actor_host.py compares training/losses.py::DDPG with the
committed file.  Cases: n_step 1, 3 and T itself (T = 9, E = 6, one agent), done flags mid-batch and on the last row, with
and without the two normalisations."""
import json
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def main():
    import torch
    from warp_drive.training.algorithms.policygradient.ddpg import DDPG

    T, E, n = 9, 6, 1
    cases = {}
    for n_step in (1, 3, T):
        for norm in (False, True):
            cases[f"n{n_step}_{'norm' if norm else 'plain'}"] = dict(
                discount_factor_gamma=0.99 if not norm else 0.9, normalize_advantage=norm, normalize_return=norm,
                n_step=n_step)
    out, meta = {}, {}
    for ci, (name, kw) in enumerate(cases.items()):
        g = torch.Generator().manual_seed(15000 + ci)
        values = torch.randn(T, E, n, generator=g, dtype=torch.float32)
        next_values = torch.randn(T - 1, E, n, generator=g, dtype=torch.float32)
        j_values = torch.randn(T, E, n, generator=g, dtype=torch.float32)
        actions = torch.randn(T, E, n, 1, generator=g, dtype=torch.float32)
        rewards = torch.randn(T, E, n, generator=g, dtype=torch.float32) * 2.0
        done = (torch.rand(T, E, generator=g) < 0.2).to(torch.int32)
        done[-1] = 0
        done[-1, ::2] = 1   # some replicas finish on the last row, some bootstrap
        done[4, 1] = 1      # and mid-batch, whatever the draw gave
        values.requires_grad_(True)
        j_values.requires_grad_(True)
        actor_loss, critic_loss, metrics = DDPG(**kw).compute_loss_and_metrics(
            timestep=100 + ci, actions_batch=actions, rewards_batch=rewards, done_flags_batch=done,
            value_functions_batch=values, next_value_functions_batch=next_values, j_functions_batch=j_values,
            perform_logging=True)
        critic_loss.backward()
        actor_loss.backward()
        out[f"{name}.values"] = values.detach().numpy()
        out[f"{name}.next_values"] = next_values.numpy()
        out[f"{name}.j_values"] = j_values.detach().numpy()
        out[f"{name}.actions"] = actions.numpy()
        out[f"{name}.rewards"] = rewards.numpy()
        out[f"{name}.done"] = done.numpy()
        out[f"{name}.grad_values"] = values.grad.numpy()
        out[f"{name}.grad_j_values"] = j_values.grad.numpy()
        out[f"{name}.actor_loss"] = np.float64(actor_loss.item())
        out[f"{name}.critic_loss"] = np.float64(critic_loss.item())
        meta[name] = {"kwargs": kw, "timestep": 100 + ci, "metrics": {k: float(v) for k, v in metrics.items()}}
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, "ddpg_loss_fixtures.npz"), **out)
    print(f"ddpg_loss_fixtures.npz: {len(cases)} cases from the reference's DDPG compute_loss_and_metrics")


if __name__ == "__main__":
    main()
