"""Actor and critic of the DDPG trainer (training/trainer_ddpg.py) for a one-dimensional `Box` action.

The reference's counterparts are warp_drive/training/models/fully_connected_actor.py and
fully_connected_action_value_critic.py: an MLP trunk with a tanh output scaled into the action range, and an MLP on the
concatenated (observation, action) with one output.  The actor's module layout -- `fc["0"]`, `fc["1"]`, `action_head` --
is the one training/policy_kernel.py::pack_rollout_actor reads, so the rollout kernels of the Box envs can evaluate it
(csrc/kernels/classic_control.hip::cc_actor_mean, the actor head of csrc/kernels/rollout_policy.h)."""
import numpy as np
import torch
from torch import nn

from warp_drive_amd.utils.spaces import Box


def box_action_range(action_space):
    """(low, high) of a one-dimensional Box action space, as Python floats"""
    if not isinstance(action_space, Box) or tuple(action_space.shape) != (1,):
        raise NotImplementedError("the DDPG trainer drives one-dimensional Box action spaces")
    return float(np.asarray(action_space.low).reshape(-1)[0]), float(np.asarray(action_space.high).reshape(-1)[0])


def actor_output_range(action_space, model_config=None):
    """(action_scale, action_bias) of the actor's output, mean = action_scale * tanh(z) + action_bias: `output_w` of the
    model's config when it gives one, else (high - low) / 2; (high + low) / 2"""
    low, high = box_action_range(action_space)
    scale = (model_config or {}).get("output_w")
    return float((high - low) / 2.0 if scale is None else scale), float((high + low) / 2.0)


class FullyConnectedActor(nn.Module):
    name = "torch_fully_connected_actor"

    def __init__(self, obs_size, fc_dims=(64, 64), action_scale=1.0, action_bias=0.0):
        super().__init__()
        dims = [int(obs_size)] + [int(d) for d in fc_dims]
        self.fc = nn.ModuleDict({
            str(i): nn.Sequential(nn.Linear(dims[i], dims[i + 1]), nn.ReLU()) for i in range(len(dims) - 1)})
        self.action_head = nn.Linear(dims[-1], 1)
        self.action_scale, self.action_bias = float(action_scale), float(action_bias)

    def forward(self, obs):
        """obs [..., obs_size] -> the actions [..., 1]"""
        x = obs
        for i in range(len(self.fc)):
            x = self.fc[str(i)](x)
        return self.action_scale * torch.tanh(self.action_head(x)) + self.action_bias


class FullyConnectedActionValueCritic(nn.Module):
    name = "torch_fully_connected_action_value_critic"

    def __init__(self, input_size, fc_dims=(64, 64)):
        """input_size = obs_size + 1: Q is evaluated on cat(obs, action)"""
        super().__init__()
        dims = [int(input_size)] + [int(d) for d in fc_dims]
        self.fc = nn.ModuleDict({
            str(i): nn.Sequential(nn.Linear(dims[i], dims[i + 1]), nn.ReLU()) for i in range(len(dims) - 1)})
        self.q_head = nn.Linear(dims[-1], 1)

    def forward(self, obs, action):
        """obs [..., obs_size], action [..., 1] -> Q [...]"""
        x = torch.cat([obs, action.to(obs.dtype)], dim=-1)
        for i in range(len(self.fc)):
            x = self.fc[str(i)](x)
        return self.q_head(x)[..., 0]
