"""DDPG for the envs with a one-dimensional `Box` action (ClassicControl Pendulum and ContinuousMountainCar): a sibling of
training/trainer.py::Trainer that shares its env wrapper, sampler, data placeholders, rollout engine, perf stats and
metric log.  The update is the framework's by default; `trainer.fused_update: true` runs it as four launches of this
repository's kernels (training/ddpg_update_kernels.py).

Mirror of the reference's warp_drive/training/trainers/trainer_ddpg.py: a deterministic actor whose output is the mean of
the OU / Gaussian exploration draw, a critic on cat(obs, action), target copies of both that follow by `tau`, n-step
returns over the rolling on-policy batch (training/losses.py::DDPG).  Single process."""
import json
import logging
import os
import time

import numpy as np
import torch
import yaml

from warp_drive_amd import distributed as wdd
from warp_drive_amd.managers.function_manager import HIPSampler
from warp_drive_amd.rollout import RolloutEngine, UnsupportedRolloutShape
from warp_drive_amd.training import ddpg_update_kernels as duk
from warp_drive_amd.training.data_loader import create_and_push_data_placeholders
from warp_drive_amd.training.losses import DDPG
from warp_drive_amd.training.models import flattened_obs_size
from warp_drive_amd.training.models_ddpg import (FullyConnectedActionValueCritic, FullyConnectedActor,
                                                 actor_output_range)
from warp_drive_amd.training.param_scheduler import ParamScheduler
from warp_drive_amd.training.policy_kernel import pack_rollout_actor, parameter_versions, rollout_actor_width
from warp_drive_amd.training.trainer import _DEFAULT_CONFIG, PerfStats, Trainer, recursive_merge_config_dicts
from warp_drive_amd.utils.constants import Constants

_OBSERVATIONS = Constants.OBSERVATIONS
_ACTIONS = Constants.ACTIONS
_REWARDS = Constants.REWARDS


def _pair(value, what):
    """a setting given once for both networks, or as {"actor": ..., "critic": ...}"""
    if isinstance(value, dict) and "actor" in value and "critic" in value:
        return value["actor"], value["critic"]
    if isinstance(value, dict) and what == "lr":
        raise ValueError("policy.*.lr: a number, a schedule, or {actor: ..., critic: ...}")
    return value, value


@torch.no_grad()
def soft_update(target, source, tau):
    """t = t * (1 - tau) + p * tau for every parameter: the expression as written (two products, one sum), over all
    parameters at once"""
    t, p = list(target.parameters()), list(source.parameters())
    torch._foreach_copy_(t, torch._foreach_add(torch._foreach_mul(t, 1.0 - tau), torch._foreach_mul(p, tau)))


@torch.no_grad()
def hard_update(target, source):
    for t, p in zip(target.parameters(), source.parameters()):
        t.copy_(p)


class TrainerDDPG:
    """One policy over all agents of the env.  Per iteration: roll out T = train_batch_size // num_envs ticks into the
    [T, E, ...] batch placeholders, then -- when the batch has a valid row: T >= max(n_step, 2) -- one critic step and one
    actor step (the T - n_step + 1 rows with n_step rows from them on are valid; the next values are T - 1 rows).

    Config (beyond Trainer's): `policy.<tag>.algorithm: "DDPG"`, `tau`, `model` ({type, fc_dims[, output_w]} for both
    networks or {actor: ..., critic: ...}), `lr` (a number, a schedule, or {actor, critic}); `trainer.n_step`;
    `sampler.params` {damping, stddev, scale} of the exploration draw (defaults 0.15 / 0.2 / 1.0).

    Rollout.  "per tick" (default): the actor's forward in the framework writes the means, the env's fused tick draws the
    action around them, steps and restarts finished replicas.  "one launch": under `trainer.fused_rollout_policy: "all"`,
    with a [32, 32] or [64, 64] actor on an env whose kernel evaluates it (`has_live_actor_rollout`) and T > 1, ONE launch
    of ...Rollout_A<width> records the whole batch; the actor is repacked in place before it.  `rollout_path` says which.

    Evaluation.  `evaluate_episodes` is "per tick" by default.  Under `trainer.fused_evaluation: true` (opt-in; absent =
    false), when the rollout is "one launch" and the env's kernel evaluates an actor of that width
    (`has_live_actor_evaluate`), ONE launch of ...Evaluate_A<width> runs the whole episode of every replica; otherwise the
    per-tick path is used and the reason is logged.  `evaluation_path` says which the last call took.
    `trainer.evaluator: true` (the reference's key; default false): every logging iteration runs a greedy
    `evaluate_episodes` -- on whichever path is available -- and adds "Mean episodic reward (test)" and "Mean episodic
    steps (test)" (the means over the replicas) to the policy's metrics.  As in the reference, that evaluation RESTARTS
    ALL ENVS at each log (`reset_all_envs()` before and after): the training rollout continues from fresh episodes, and
    the running per-episode reward accumulators are cleared.

    Update.  DELIBERATE DEPARTURE from the reference: it calls `actor_loss.backward()` and `critic_loss.backward()` on one
    graph, so the gradient of -Q(obs, actor(obs)) with respect to the CRITIC's parameters is added to the critic's
    gradient, and the critic is partly trained to raise its own output.  Here the critic's step uses the critic loss
    alone and the actor's step differentiates -Q(obs, actor(obs)) with respect to the actor's parameters only (standard
    DDPG).  Values, losses and metrics are otherwise the reference's.
    "framework" (default): autograd, `clip_grad_norm_`, two `torch.optim.Adam`s, `soft_update` -- about 150 small ops.
    "kernels": under `trainer.fused_update: true` (opt-in; absent from the run's own config = false: the `True` that
    default_configs.yaml gives the key is Trainer's A2C / PPO default and is not read here), for one agent, an actor and
    a critic of two hidden layers of one width in {32, 64}, observations of 2 or 3 floats and `normalize_return: false`
    (`ddpg_update_kernels.admitted_shape`; anything else logs the reason and uses the framework path): FOUR launches --
    next values; n-step returns + both gradients as per-block partials; reduce; clip + Adam + soft update + the packed
    actor's refill -- with nothing read back on a non-logging iteration.  The parameters of the actor and the critic, and
    of the two targets, are then views of one flat buffer each (`FlatNetworks`), which the kernels update in place: the
    modules stay the source of truth for `state_dict()` and the checkpoints; Adam's moments and step count live on the
    trainer (`_adam`).  `fused_update: "all"` (Trainer's opt-in for its own kernels path) means `true` here.  After the
    Apply launch has refilled the packed actor the one-launch rollout skips its framework-side repack for as long as the
    actor's version counters stand.  A logging iteration computes the framework path's metrics under `no_grad` from the networks
    before the step, with the gradient norms from the reduce launch.  Works with either rollout path.  `update_path`
    says which."""

    update_path = "framework"
    _update_kernels = None   # training/ddpg_update_kernels.py::DdpgUpdateKernels on the "kernels" path

    def __init__(self, env_wrapper=None, config=None, policy_tag_to_agent_id_map=None, device_id=0, results_dir=None,
                 verbose=True):
        assert env_wrapper is not None and env_wrapper.env_backend == "hip"
        assert config is not None and "trainer" in config and "policy" in config
        self.w, self.verbose = env_wrapper, verbose
        self.rank, _, self.world = wdd.rank_info()
        if self.world > 1:
            raise NotImplementedError("TrainerDDPG runs in a single process")
        self.device = torch.device("cuda", device_id)
        # (read before the defaults are merged in: default_configs.yaml's `fused_update: True` is Trainer's A2C / PPO key)
        wants_update_kernels = config["trainer"].get("fused_update", False)
        if isinstance(wants_update_kernels, str) and wants_update_kernels != "all":
            raise ValueError(f"trainer.fused_update: True, False or \"all\", not {wants_update_kernels!r}")
        wants_update_kernels = bool(wants_update_kernels)   # ("all" = true here)
        defaults = yaml.safe_load(open(_DEFAULT_CONFIG))
        for key, default in defaults.items():
            if key == "policy":
                for pol in config["policy"]:
                    recursive_merge_config_dicts(config["policy"][pol], default)
            else:
                config[key] = recursive_merge_config_dicts(config.get(key, {}), default)
        self.config = config
        E, N = env_wrapper.n_envs, env_wrapper.n_agents
        if policy_tag_to_agent_id_map is None:
            policy_tag_to_agent_id_map = {"shared": list(range(N))}
        self.policy_map = {k: list(v) for k, v in policy_tag_to_agent_id_map.items()}
        self.policies = list(self.policy_map)
        if len(self.policies) != 1 or self.policy_map[self.policies[0]] != list(range(N)):
            raise NotImplementedError("TrainerDDPG trains one policy shared by all agents")
        pol = self.policies[0]
        assert set(config["policy"]) == {pol}, "every policy needs a config entry"
        tcfg, pcfg = config["trainer"], config["policy"][pol]
        if str(pcfg["algorithm"]).upper() != "DDPG":
            raise NotImplementedError(f"algorithm {pcfg['algorithm']}: TrainerDDPG trains DDPG (A2C / PPO: Trainer)")
        self.num_envs = E
        self.batch_len = max(1, int(tcfg["train_batch_size"]) // E)
        self.train_batch_size = self.batch_len * E
        self.num_iters = int(tcfg["num_episodes"]) * env_wrapper.episode_length // self.train_batch_size
        if self.num_iters == 0:
            raise ValueError("Not enough steps to even perform a single training iteration!. Please increase the "
                             "number of episodes or reduce the training batch size.")
        self.n_step = int(tcfg.get("n_step", 1))
        self.tau = float(pcfg.get("tau", 0.05))
        self.save_dir = results_dir or os.path.join(config["saving"]["basedir"], config["saving"]["name"],
                                                    config["saving"]["tag"], str(int(time.time())))
        os.makedirs(self.save_dir, exist_ok=True)
        json.dump(config, open(os.path.join(self.save_dir, "run_config.json"), "w"), indent=2, default=str)

        # ---- device data (as Trainer)
        seed = tcfg.get("seed", 0) or 0
        env_wrapper.reset_all_envs()
        if len(env_wrapper.cuda_data_manager.reset_target_to_pool):
            env_wrapper.init_reset_pool(wdd.rank_seed(seed, self.rank))
        self.sampler = HIPSampler(env_wrapper.cuda_function_manager)
        self.sampler.init_random(seed=wdd.rank_seed(seed, self.rank) + 1)
        create_and_push_data_placeholders(env_wrapper=env_wrapper, action_sampler=self.sampler,
                                          policy_tag_to_agent_id_map=self.policy_map,
                                          training_batch_size_per_env=self.batch_len, push_data_batch_placeholders=True)
        dm = env_wrapper.cuda_data_manager
        self.obs = dm.data_on_device_via_torch(_OBSERVATIONS)
        self.actions = dm.data_on_device_via_torch(_ACTIONS)
        self.rewards = dm.data_on_device_via_torch(_REWARDS)
        self.done = dm.data_on_device_via_torch("_done_")
        self.done_batch = dm.data_on_device_via_torch(f"{Constants.DONE_FLAGS}_batch")
        space = env_wrapper.env.action_space[0]
        obs_size = flattened_obs_size(env_wrapper.env.observation_space[0])
        self.batch = {pol: {
            "obs": dm.data_on_device_via_torch(f"{Constants.PROCESSED_OBSERVATIONS}_batch_{pol}") if self.batch_len > 1
            else torch.zeros((1, E, N, obs_size), device=self.device),
            "actions": dm.data_on_device_via_torch(f"{_ACTIONS}_batch_{pol}"),
            "rewards": dm.data_on_device_via_torch(f"{_REWARDS}_batch_{pol}")}}
        self.ids = {pol: torch.arange(N, device=self.device)}

        # ---- networks, targets, optimisers, objective
        actor_cfg, critic_cfg = _pair(pcfg["model"], "model")
        scale, bias = actor_output_range(space, actor_cfg)
        self.actors = {pol: FullyConnectedActor(obs_size, actor_cfg["fc_dims"], scale, bias).to(self.device)}
        self.critics = {pol: FullyConnectedActionValueCritic(obs_size + 1, critic_cfg["fc_dims"]).to(self.device)}
        self.target_actors = {pol: FullyConnectedActor(obs_size, actor_cfg["fc_dims"], scale, bias).to(self.device)}
        self.target_critics = {pol: FullyConnectedActionValueCritic(obs_size + 1, critic_cfg["fc_dims"]).to(self.device)}
        self.models = self.actors  # (what Trainer's shared rollout bookkeeping repacks)
        self.current_timestep = {pol: 0}
        ckpt = actor_cfg.get("model_ckpt_filepath", "")
        if isinstance(ckpt, dict) and ckpt.get("actor") and ckpt.get("critic"):
            self.load_model_checkpoint({pol: ckpt})
        else:
            hard_update(self.target_actors[pol], self.actors[pol])
            hard_update(self.target_critics[pol], self.critics[pol])
        for net in (self.target_actors[pol], self.target_critics[pol]):
            for p in net.parameters():
                p.requires_grad_(False)
        actor_lr, critic_lr = _pair(pcfg["lr"], "lr")
        self.lr_schedules = {pol: (ParamScheduler(actor_lr), ParamScheduler(critic_lr))}
        # (on the "kernels" update path these two are never stepped and their state stays empty: Adam's moments and step
        # count are then `self._adam`)
        self.actor_optimizers = {pol: torch.optim.Adam(self.actors[pol].parameters(),
                                                       lr=self.lr_schedules[pol][0].get_param_value(0))}
        self.critic_optimizers = {pol: torch.optim.Adam(self.critics[pol].parameters(),
                                                        lr=self.lr_schedules[pol][1].get_param_value(0))}
        self.trainers = {pol: DDPG(discount_factor_gamma=pcfg["gamma"], normalize_advantage=pcfg["normalize_advantage"],
                                   normalize_return=pcfg["normalize_return"], n_step=self.n_step)}

        # ---- update: the framework's ops, or -- when asked for and the shape is admitted -- the four update launches
        if wants_update_kernels:
            ok, why = duk.admitted_shape(len(self.policies), N, obs_size, int(np.prod(space.shape)), actor_cfg["fc_dims"],
                                         critic_cfg["fc_dims"], bool(pcfg["normalize_return"]))
            if ok and self.batch_len < max(self.n_step, 2):
                ok, why = False, f"a batch of {self.batch_len} rows has no valid row for n_step {self.n_step}"
            if ok:
                self._flat = duk.FlatNetworks(self.actors[pol], self.critics[pol])
                self._flat_target = duk.FlatNetworks(self.target_actors[pol], self.target_critics[pol])
                self._adam = {"step": 0, "exp_avg": torch.zeros_like(self._flat.flat),
                              "exp_avg_sq": torch.zeros_like(self._flat.flat)}
                self._update_kernels = duk.DdpgUpdateKernels(env_wrapper.cuda_function_manager, E, self.batch_len,
                                                             self.n_step, self._flat.H, obs_size, self.device)
                self._actor_range = (scale, bias)
                self.update_path = "kernels"
            else:
                duk.log_refusal(why)

        # ---- rollout: the means the tick reads, the single-tick engine, and -- when asked for -- the one-launch engine
        params = dict((config.get("sampler") or {}).get("params") or {})
        self.ou_params = {"damping": float(params.get("damping", 0.15)), "stddev": float(params.get("stddev", 0.2)),
                          "scale": float(params.get("scale", 1.0))}
        self.means = torch.zeros((E, N, 1), dtype=torch.float32, device=self.device)
        self.engine = RolloutEngine(env_wrapper, self.sampler, probabilities=[self.means], reset_done=True,
                                    ticks_per_launch=1, **self.ou_params)
        if not self.engine.fused:
            raise UnsupportedRolloutShape(f"{type(env_wrapper.env).__name__} has no fused tick: TrainerDDPG needs one")
        self._greedy_engine = None
        self._batch_rollout = None
        self.rollout_path = "per tick"
        wanted = tcfg.get("fused_rollout_policy", True)
        if isinstance(wanted, str) and wanted != "all":
            raise ValueError(f"trainer.fused_rollout_policy: True, False or \"all\", not {wanted!r}")
        width = rollout_actor_width(self.actors[pol], obs_size, getattr(env_wrapper.env, "ROLLOUT_ACTOR_WIDTHS", ()))
        if wanted == "all" and width is not None and self.batch_len > 1 and N == 1:
            packed = pack_rollout_actor(self.actors[pol]).to(self.device)
            env_batch = {"obs": self.batch[pol]["obs"], "actions": self.batch[pol]["actions"],
                         "rewards": self.batch[pol]["rewards"], "done": self.done_batch}
            try:
                self._batch_engine = RolloutEngine(env_wrapper, self.sampler, probabilities=[self.means], reset_done=True,
                                                   rollout_batch=env_batch, rollout_actor=(packed, width, scale, bias),
                                                   ticks_per_launch=self.batch_len, **self.ou_params)
                self._batch_rollout = {"packed": {pol: packed}, "pack": pack_rollout_actor, "split": None,
                                       "width": width, "range": (scale, bias)}
                self.rollout_path = "one launch"
            except UnsupportedRolloutShape as err:
                logging.info(f"whole-batch rollout not available for this shape ({err}); using the per-tick path")
        if tcfg.get("fused_evaluation", False) and self._one_launch_evaluation() is None:
            logging.info("trainer.fused_evaluation: no one-launch evaluation for this shape (it needs the one-launch "
                         "rollout and an Evaluate_A entry of the actor's width); evaluate_episodes uses the per-tick path")

        # ---- episodic reward bookkeeping, all on the device (as Trainer)
        self._ep_reward = {pol: torch.zeros((E, N), device=self.device)}
        self._ep_sum = {pol: torch.zeros(E, device=self.device)}
        self._ep_cnt = torch.zeros(E, device=self.device)
        self.perf_stats = PerfStats()
        self.metrics = {}

    # --------------------------------------------------------------------------- rollout
    @torch.no_grad()
    def _tick(self, t):
        """actor forward -> the means; the env's fused tick (OU draw, step, restart); row t of the batch"""
        pol = self.policies[0]
        batch = self.batch[pol]
        batch["obs"][t].copy_(self.obs.reshape(batch["obs"].shape[1:]))
        self.means.copy_(self.actors[pol](batch["obs"][t]))
        self.engine.run(1)
        self.done_batch[t].copy_(self.done)
        batch["actions"][t].copy_(self.actions)
        batch["rewards"][t].copy_(self.rewards)
        finished = (self.done > 0).to(torch.float32)
        self._ep_reward[pol] += self.rewards
        self._ep_sum[pol] += self._ep_reward[pol].mean(dim=1) * finished
        self._ep_reward[pol] *= (1.0 - finished)[:, None]
        self._ep_cnt += finished

    # the whole batch as one launch, then the episodic bookkeeping vectorised over the recorded rows: Trainer's own code
    # (it repacks `self.models` = the actors through `_batch_rollout["pack"]` and runs `self.engine` once)
    _bookkeep_one_launch = Trainer._generate_rollout_batch_in_one_launch

    def _generate_rollout_batch(self):
        if self._batch_rollout is not None:
            per_tick, self.engine = self.engine, self._batch_engine
            try:
                self._bookkeep_one_launch()
            finally:
                self.engine = per_tick
            return
        for t in range(self.batch_len):
            self._tick(t)

    # ---------------------------------------------------------------------------- update
    def _update_model_params(self, iteration, log):
        if self._update_kernels is not None:
            return self._update_with_kernels(log)
        pol = self.policies[0]
        pcfg = self.config["policy"][pol]
        T = self.batch_len
        metrics = {pol: {"Total loss": float("nan")}} if log else {}
        actor_lr = critic_lr = actor_norm = critic_norm = 0.0
        if pcfg["to_train"] and T >= max(self.n_step, 2):
            actor, critic = self.actors[pol], self.critics[pol]
            obs, actions = self.batch[pol]["obs"][:T], self.batch[pol]["actions"][:T]
            with torch.no_grad():
                next_values = self.target_critics[pol](obs[1:], self.target_actors[pol](obs[1:]))
            values = critic(obs, actions)
            j_values = critic(obs, actor(obs))
            self.current_timestep[pol] += self.train_batch_size
            actor_loss, critic_loss, m = self.trainers[pol].compute_loss_and_metrics(
                self.current_timestep[pol], actions, self.batch[pol]["rewards"][:T], self.done_batch[:T], values,
                next_values, j_values, perform_logging=log)
            a_params, c_params = list(actor.parameters()), list(critic.parameters())
            # (each loss differentiated with respect to its own network only: see the class docstring)
            c_grads = torch.autograd.grad(critic_loss, c_params, retain_graph=True)
            a_grads = torch.autograd.grad(actor_loss, a_params)
            for params, grads in ((a_params, a_grads), (c_params, c_grads)):
                for p, g in zip(params, grads):
                    p.grad = g
            actor_lr = self.lr_schedules[pol][0].get_param_value(self.current_timestep[pol])
            critic_lr = self.lr_schedules[pol][1].get_param_value(self.current_timestep[pol])
            for opt, lr in ((self.actor_optimizers[pol], actor_lr), (self.critic_optimizers[pol], critic_lr)):
                for group in opt.param_groups:
                    group["lr"] = lr
            if log:
                actor_norm = float(sum(g.norm(2) for g in a_grads))
                critic_norm = float(sum(g.norm(2) for g in c_grads))
            if pcfg["clip_grad_norm"]:
                torch.nn.utils.clip_grad_norm_(a_params, pcfg["max_grad_norm"])
                torch.nn.utils.clip_grad_norm_(c_params, pcfg["max_grad_norm"])
            self.actor_optimizers[pol].step()
            self.critic_optimizers[pol].step()
            soft_update(self.target_actors[pol], actor, self.tau)
            soft_update(self.target_critics[pol], critic, self.tau)
            if log:
                metrics[pol] = m
        if log:
            self._add_common_metrics(metrics[pol], pol, actor_norm, critic_norm, actor_lr, critic_lr)
        return metrics

    def _add_common_metrics(self, m, pol, actor_norm, critic_norm, actor_lr, critic_lr):
        cnt = float(self._ep_cnt.sum().item())
        m.update({
            "Current timestep": self.current_timestep[pol], "Gradient norm (Actor)": actor_norm,
            "Gradient norm (Critic)": critic_norm, "Learning rate (Actor)": actor_lr,
            "Learning rate (Critic)": critic_lr,
            "Mean episodic reward": float(self._ep_sum[pol].sum().item()) / cnt if cnt > 0 else float("nan")})

    def _update_with_kernels(self, log):
        """`_update_model_params` as four launches (see the class docstring); a non-logging iteration reads nothing back"""
        pol = self.policies[0]
        pcfg = self.config["policy"][pol]
        T, k = self.batch_len, self._update_kernels
        metrics = {pol: {"Total loss": float("nan")}} if log else {}
        actor_lr = critic_lr = actor_norm = critic_norm = 0.0
        if pcfg["to_train"] and T >= max(self.n_step, 2):
            assert self._flat.bound() and self._flat_target.bound(), "a parameter's .data was re-assigned"
            obs, actions = self.batch[pol]["obs"][:T], self.batch[pol]["actions"][:T]
            rewards, done = self.batch[pol]["rewards"][:T], self.done_batch[:T]
            self.current_timestep[pol] += self.train_batch_size
            if log:  # the framework path's metrics, from the networks before the step
                with torch.no_grad():
                    next_values = self.target_critics[pol](obs[1:], self.target_actors[pol](obs[1:]))
                    values = self.critics[pol](obs, actions)
                    j_values = self.critics[pol](obs, self.actors[pol](obs))
                    _, _, metrics[pol] = self.trainers[pol].compute_loss_and_metrics(
                        self.current_timestep[pol], actions, rewards, done, values, next_values, j_values,
                        perform_logging=True)
            actor_lr = self.lr_schedules[pol][0].get_param_value(self.current_timestep[pol])
            critic_lr = self.lr_schedules[pol][1].get_param_value(self.current_timestep[pol])
            scale, bias = self._actor_range
            k.targets(obs, self._flat_target.flat, scale, bias)
            k.gradients(obs, actions, rewards, done, k.next_values, self._flat.flat, pcfg["gamma"], scale, bias)
            k.reduce()
            if log:
                actor_norm, critic_norm = k.gradient_norms()
            self._adam["step"] += 1
            packed = self._batch_rollout["packed"][pol] if self._batch_rollout is not None else None
            k.apply(self._flat.flat, self._flat_target.flat, self._adam["exp_avg"], self._adam["exp_avg_sq"],
                    self._adam["step"], actor_lr, critic_lr, self.tau,
                    max_norm=pcfg["max_grad_norm"] if pcfg["clip_grad_norm"] else None, packed=packed)
            if packed is not None:  # (the rollout skips its repack while the actor's version counters stay as they are)
                self._batch_rollout.setdefault("refilled", {})[pol] = parameter_versions(self.actors[pol])
        if log:
            self._add_common_metrics(metrics[pol], pol, actor_norm, critic_norm, actor_lr, critic_lr)
        return metrics

    # ----------------------------------------------------------------------------- train
    train = Trainer.train
    graceful_close = Trainer.graceful_close

    def _evaluator_metrics(self):
        """the reference's test evaluator: one greedy (noise-free) `evaluate_episodes`, its means over the replicas"""
        rewards, steps = self.evaluate_episodes(use_argmax=True)
        return {pol: {"Mean episodic reward (test)": float(rewards[pol].mean()),
                      "Mean episodic steps (test)": float(steps[pol].mean())} for pol in self.policies}

    def _log_metrics(self, iteration, metrics):
        if self.config["trainer"].get("evaluator", False):
            for pol, test in self._evaluator_metrics().items():
                metrics[pol].update(test)
        Trainer._log_metrics(self, iteration, metrics)

    # ------------------------------------------------------------------------ checkpoints
    def _networks(self, pol):
        return {"actor": self.actors[pol], "critic": self.critics[pol], "target_actor": self.target_actors[pol],
                "target_critic": self.target_critics[pol]}

    def save_model_checkpoint(self):
        """`{policy}_{network}_{timestep}.state_dict` for the actor, the critic and both targets; returns
        {policy: {network: path}}, which `load_model_checkpoint` takes"""
        out = {}
        for pol in self.policies:
            out[pol] = {}
            for name, net in self._networks(pol).items():
                path = os.path.join(self.save_dir, f"{pol}_{name}_{self.current_timestep[pol]}.state_dict")
                state = net.state_dict()
                if self.update_path == "kernels":  # (views of the flat buffer: save each tensor's own floats only)
                    state = type(state)((key, v.detach().clone()) for key, v in state.items())
                torch.save(state, path)
                out[pol][name] = path
        return out

    def load_model_checkpoint(self, ckpts_dict):
        """ckpts_dict = {policy: {"actor": path, "critic": path[, "target_actor": path, "target_critic": path]}}; a
        target that is not given becomes a copy of its network.  The timestep is parsed from the actor's file name."""
        for pol, paths in ckpts_dict.items():
            nets = self._networks(pol)
            for name in ("actor", "critic"):
                assert os.path.isfile(paths[name]), f"invalid model checkpoint path {paths[name]}"
                nets[name].load_state_dict(torch.load(paths[name], map_location=self.device))
            for name in ("target_actor", "target_critic"):
                if paths.get(name):
                    nets[name].load_state_dict(torch.load(paths[name], map_location=self.device))
                else:
                    hard_update(nets[name], nets[name[len("target_"):]])
            stem = os.path.basename(paths["actor"]).split(".state_dict")[0]
            try:
                self.current_timestep[pol] = int(stem.split("_")[-1])
            except ValueError:
                pass

    # ------------------------------------------------------------------- evaluate_episodes
    _evaluate_accumulate_launch = Trainer._evaluate_accumulate_launch

    def _one_launch_evaluation(self):
        """(env, width) when `evaluate_episodes` is one launch: `trainer.fused_evaluation` is true, the training rollout is
        one launch (so the packed actor and its width exist) and the env has an Evaluate_A entry of that width; else None"""
        br = self._batch_rollout
        if not self.config["trainer"].get("fused_evaluation", False) or self.rollout_path != "one launch" or br is None:
            return None
        env = self.w.env
        if not hasattr(env, "has_live_actor_evaluate") or not env.has_live_actor_evaluate(br["width"]):
            return None
        return env, br["width"]

    @torch.no_grad()
    def evaluate_episodes(self, **sample_params):
        """Trainer.evaluate_episodes' contract (points 1 to 7 of its docstring, the same return types).  `use_argmax=True`
        (greedy): the action is the actor's mean -- exploration scale 0, which draws nothing and leaves the sampler's RNG
        words and the OU state untouched; otherwise the training rollout's exploration noise (`ou_params`).
        "one launch" (`_one_launch_evaluation`): the actor is repacked in place into the tensor the rollout owns and one
        ...Evaluate_A<width> launch runs every replica's episode; it reads the env's arrays only, so they stay as
        `reset_all_envs()` left them.  "per tick": actor forward -> means, one fused tick (greedy: a second engine built
        with scale 0), HipEvaluateAccumulate on `rewards` / `_done_`, `episode_length` times, one all-finished check every
        32 ticks."""
        use_argmax = bool(sample_params.get("use_argmax", False))
        pol = self.policies[0]
        E, N, T = self.num_envs, self.w.n_agents, int(self.w.episode_length)
        one = self._one_launch_evaluation()
        if one is not None:
            env, width = one
            br = self._batch_rollout
            self.w.reset_all_envs()
            br["pack"](self.actors[pol], out=br["packed"][pol])  # the current weights
            ou = (self.ou_params["damping"], self.ou_params["stddev"], 0.0 if use_argmax else self.ou_params["scale"])
            out = {"reward_sum": torch.zeros((E, N), dtype=torch.float32, device=self.device),
                   "steps": torch.zeros(E, dtype=torch.int32, device=self.device),
                   "done": torch.zeros(E, dtype=torch.int32, device=self.device)}
            fn, args, block, grid, shared = env.evaluate_actor_launch(
                self.sampler, actor=(br["packed"][pol], width, *br["range"]), ou=ou, outputs=out, ticks=T)
            fn(*args, block=block, grid=grid, shared=shared)
            steps = out["steps"].cpu().numpy().astype(np.int32)
            assert (out["done"].cpu().numpy() != 0).all(), "a replica did not finish within episode_length ticks"
            self.evaluation_path = "one launch"
            self._ep_reward[pol].zero_()
            return ({pol: np.ascontiguousarray(out["reward_sum"].cpu().numpy().reshape(E, N), dtype=np.float32)},
                    {pol: steps.copy()})
        if use_argmax and self._greedy_engine is None:
            self._greedy_engine = RolloutEngine(self.w, self.sampler, probabilities=[self.means], reset_done=True,
                                                ticks_per_launch=1, **{**self.ou_params, "scale": 0.0})
        engine = self._greedy_engine if use_argmax else self.engine
        self.w.reset_all_envs()
        reward_sum = torch.zeros((E, N), dtype=torch.float32, device=self.device)
        end_tick = torch.full((E,), -1, dtype=torch.int32, device=self.device)
        for k in range(T):
            self.means.copy_(self.actors[pol](self.obs.reshape(E, N, -1)))
            engine.run(1)
            fn, args, block, grid, shared = self._evaluate_accumulate_launch(reward_sum, end_tick, k)
            fn(*args, block=block, grid=grid, shared=shared)
            if (k + 1) % 32 == 0 and k + 1 < T and bool((end_tick >= 0).all()):
                break
        steps = (end_tick.cpu().numpy() + 1).astype(np.int32)
        assert (steps > 0).all(), "a replica did not finish within episode_length ticks"
        self.w.reset_all_envs()
        self.evaluation_path = "per tick"
        self._ep_reward[pol].zero_()
        return ({pol: np.ascontiguousarray(reward_sum.cpu().numpy(), dtype=np.float32)},
                {pol: steps.copy()})
