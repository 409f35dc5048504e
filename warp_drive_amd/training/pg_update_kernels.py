"""Trainer's A2C / PPO update for the in-kernel policies as five launches (csrc/kernels/pg_update.hip, code object
wd_kernels_pg.hsaco; the returns entry is wd_kernels_update.hsaco's):

    HipPgValues_H<H>_O<O>     values [T, E] of the recorded rows
    HipDiscountedReturns      the existing entry on `values` (w = 1, v_col = 0): returns and advantages [T, E]
    HipPgGradients_H<H>_O<O>  forward, the objective's gradient, backward: one partial of the eight tensors per block
    HipPgReduce               partials -> flat gradient, per-tensor sums of squares, the four sums of the objective
    HipPgApply                clip, Adam, refill of the rollout's packed policy

`trainer.fused_update: "all"` selects it (opt-in; training/trainer.py).  `trainer.fused_update_gradients: "matrix"` then
launches HipPgGradientsMx_H<H>_O<O> (csrc/kernels/pg_update_matrix.hip, wd_kernels_pg_mx.hsaco) in the third place: the
same arguments and partials, the three H x H products per row on the float32 matrix cores.
`trainer.fused_update_normalize: true` serves a policy with `normalize_return` / `normalize_advantage` too: two or three
launches of csrc/kernels/pg_normalize.hip (wd_kernels_pg_norm.hsaco) between the second and the third
(`_PgUpdateLaunches.normalize`).  `admitted_shape` says which policies it serves;
`trainer.fused_update_downsample: true` serves `trainer.neg_pos_env_ratio` too: three launches of
csrc/kernels/pg_downsample.hip (wd_kernels_pg_select.hsaco) before the first, one read-back of three integers, and
the launches above on the kept columns (`_PgUpdateLaunches.downsample`).
A policy with `gae_lambda` launches HipPgGaeReturns (csrc/kernels/pg_gae.hip, wd_kernels_pg_gae.hsaco) in the second place:
GAE(lambda) advantages as a scan over time, returns = advantages + values (`_PgUpdateLaunches.gae_returns`).
`PgUpdateKernels` holds the launch wrappers, their geometry fixed from E, T, H, O, A and the compute-unit count;
`FlatPolicy` makes the parameters of a FullyConnected views of one flat float32 buffer in the kernels' layout, so the
kernels update the module in place and the module remains the source of truth.

Layout (the order of the module's parameters): W0 [H][O], b0 [H], W1 [H][H], b1 [H], Wp [A][H], bp [A], Wv [1][H], bv [1].
Its first six tensors are pack_rollout_policy's layout."""
import logging

import numpy as np
import torch

HIDDEN = (32, 64)          # widths the code object has entries for
OBS_SIZES = (2, 4, 6)      # MountainCar, Cartpole, Acrobot
MAX_ACTIONS = 8
TILE = 128                 # rows per tile = threads per block of HipPgGradients (its __launch_bounds__)
LD = TILE + 4              # row stride of the arrays it stages in LDS
VALUES_MAX_THREADS = 256   # __launch_bounds__ of HipPgValues
RETURNS_THREADS = 256      # __launch_bounds__ of HipDiscountedReturns
REDUCE_THREADS = 1024      # block size HipPgReduce is written for
TENSORS = 8
REDUCE_BLOCKS = TENSORS + 1   # eight parameter tensors + the four sums
SUMS = 4                   # sum logp * adv, sum entropy, sum (v - ret)^2, sum adv
APPLY_THREADS = 256
LDS_LIMIT = 160 * 1024
GRADIENTS_ENTRIES = ("lanes", "matrix")   # HipPgGradients (one row per lane) | HipPgGradientsMx (the matrix cores)
MATRIX_THREADS = 256       # __launch_bounds__ of HipPgGradientsMx: four wavefronts of 32 rows, the same 128-row tile
MATRIX_LD = 36             # row stride of the arrays a wavefront stages ([unit][32 rows])
MATRIX_MAX_OBS = 6
MATRIX_BLOCKS_PER_CU = {32: 2, 64: 1}   # what registers and LDS let a compute unit hold (docs/rounds/r47.md)
RETURNS_ENTRY = "HipDiscountedReturns"
# normalize_return / normalize_advantage between the returns and the gradient launch (csrc/kernels/pg_normalize.hip)
NORMALIZE_CODE_OBJECT = "wd_kernels_pg_norm.hsaco"
NORMALIZE_ENTRIES = ("HipPgTickMoments", "HipPgNormalizeReturns", "HipPgNormalizeAdvantages")
NORMALIZE_THREADS = 256    # their __launch_bounds__: one block per (tick, chunk), 16 columns per lane
NORMALIZE_CHUNK = 16 * NORMALIZE_THREADS
NORMALIZE_EPS = 1.0e-10    # losses._EPSILON
# neg_pos_env_ratio before the values launch (csrc/kernels/pg_downsample.hip)
DOWNSAMPLE_CODE_OBJECT = "wd_kernels_pg_select.hsaco"
DOWNSAMPLE_ENTRIES = ("HipPgSelectScan", "HipPgSelectKeep", "HipPgGatherColumns")
SELECT_SCAN_THREADS = 256  # one lane per replica
SELECT_KEEP_THREADS = 1024  # HipPgSelectKeep is ONE block of these
GATHER_THREADS = 256
GATHER_CHUNK = 256         # kept columns per block of HipPgGatherColumns
DOWNSAMPLE_STREAM_TAG = 0x646F776E   # "down": counter word 2 of the keys' Philox stream (word 3 is 6)
# GAE(lambda) in the returns launch's position (csrc/kernels/pg_gae.hip; the policy key `gae_lambda`)
GAE_CODE_OBJECT = "wd_kernels_pg_gae.hsaco"
GAE_ENTRY = "HipPgGaeReturns"
GAE_TILE = 64              # columns of a block: one per lane
GAE_WAVEFRONTS = (1, 2, 4, 8, 16)   # S, the wavefronts of a block: each owns ceil(T / S) consecutive ticks
GAE_MIN_ROWS = 8           # a segment shorter than this is not worth a wavefront
GAE_FULL_DEVICE = 4        # tiles per compute unit (one wavefront per SIMD) from which time is not split
_NULL = np.uint64(0)


def net_floats(H, O, A):
    return H * O + H + H * H + H + A * H + A + H + 1


def packed_floats(H, O, A):
    """pack_rollout_policy's tensor: everything but the value head"""
    return net_floats(H, O, A) - H - 1


def _pad4(n):
    return (n + 3) & ~3


def tensor_slices(H, O, A):
    """(offset, shape) of the eight parameter tensors inside the flat buffer"""
    out, at = [], 0
    for shape in ((H, O), (H,), (H, H), (H,), (A, H), (A,), (1, H), (1,)):
        out.append((at, shape))
        at += int(np.prod(shape))
    assert at == net_floats(H, O, A)
    return out


def values_lds_bytes(H, O):
    """the network's copy in LDS: eight head rows and eight bias slots whatever A is (the value head then starts on a
    16-byte boundary)"""
    return 4 * _pad4(net_floats(H, O, MAX_ACTIONS))


def gradients_lds_bytes(H, O):
    return values_lds_bytes(H, O) + 4 * (2 * H * LD + O * LD + (MAX_ACTIONS + 1) * LD + SUMS * LD)


def gradients_matrix_lds_bytes(H, O):
    """PgmLds<H, O>::TOTAL of pg_update_matrix.hip: the network (eight head rows, W1 with its rows padded by 8), per
    wavefront two staged arrays [H][36] and the staged inputs [6][32] and deltas [9][32]"""
    net = _pad4(H * O + H + H + MAX_ACTIONS * H + MAX_ACTIONS + H + 1) + H * (H + 8)
    return 4 * (net + (MATRIX_THREADS // 64) * (2 * H * MATRIX_LD + (MATRIX_MAX_OBS + MAX_ACTIONS + 1) * 32))


def gradients_entry_name(H, O, gradients_entry="lanes"):
    assert gradients_entry in GRADIENTS_ENTRIES, gradients_entry
    return f"HipPgGradients{'Mx' if gradients_entry == 'matrix' else ''}_H{H}_O{O}"


def kernel_names(H, O, gradients_entry="lanes"):
    """the five launches, in order"""
    return [f"HipPgValues_H{H}_O{O}", RETURNS_ENTRY, gradients_entry_name(H, O, gradients_entry), "HipPgReduce", "HipPgApply"]


def all_kernel_names():
    """every entry of wd_kernels_pg.hsaco"""
    return sorted({n for H in HIDDEN for O in OBS_SIZES for n in kernel_names(H, O)} - {RETURNS_ENTRY})


def matrix_kernel_names():
    """every entry of wd_kernels_pg_mx.hsaco"""
    return sorted(gradients_entry_name(H, O, "matrix") for H in HIDDEN for O in OBS_SIZES)


def gae_kernel_names():
    """every entry of wd_kernels_pg_gae.hsaco"""
    return [GAE_ENTRY]


def gae_wavefronts(columns, T, compute_units):
    """S of HipPgGaeReturns for a [T][columns] batch: 1 when the ceil(columns / 64) one-wavefront blocks already give
    every SIMD of the device a wavefront (GAE_FULL_DEVICE tiles per compute unit) or T is short; else the largest S of
    GAE_WAVEFRONTS that leaves every wavefront at least GAE_MIN_ROWS ticks (T // S >= GAE_MIN_ROWS)."""
    columns, T, compute_units = int(columns), int(T), int(compute_units)
    assert columns >= 1 and T >= 1 and compute_units >= 1, (columns, T, compute_units)
    if -(-columns // GAE_TILE) >= GAE_FULL_DEVICE * compute_units:
        return 1
    return max(S for S in GAE_WAVEFRONTS if S == 1 or T // S >= GAE_MIN_ROWS)


def gae_lambda_refusal(value):
    """"" when `value` is a policy's `gae_lambda` -- None or a number in [0, 1] -- else what is wrong with it"""
    if value is None or (isinstance(value, (int, float)) and not isinstance(value, bool) and 0 <= value <= 1):
        return ""
    return f"None or a number in [0, 1], not {value!r}"


def _admitted_tail(fc_dims, obs_size, obs_sizes, obs_takes, dtype, normalize_return, normalize_advantage, neg_pos_env_ratio,
                   world_size, algorithm, one_launch_rollout):
    """the checks both admission functions end with, in their order; `obs_sizes` are the observation sizes of the caller's
    kernels and `obs_takes` its words for them"""
    dims = [int(d) for d in fc_dims]
    if len(dims) != 2:
        return False, f"{len(dims)} hidden layers: the update kernels take two"
    if dims[0] != dims[1]:
        return False, f"the hidden layers have unequal widths {dims}"
    if dims[0] not in HIDDEN:
        return False, f"hidden width {dims[0]}: the update kernels exist for {list(HIDDEN)}"
    if int(obs_size) not in obs_sizes:
        return False, f"observation size {obs_size}: {obs_takes}"
    if dtype != torch.float32:
        return False, f"{dtype}: the update kernels are float32"
    if normalize_return:
        return False, "normalize_return: the returns are normalised by the framework path only"
    if normalize_advantage:
        return False, "normalize_advantage: the advantages are normalised by the framework path only"
    if neg_pos_env_ratio > 0:
        return False, "neg_pos_env_ratio: the replicas are down-sampled by the framework path only"
    if world_size != 1:
        return False, f"{world_size} ranks: the update kernels run in a single process"
    if str(algorithm).upper() not in ("A2C", "PPO"):
        return False, f"algorithm {algorithm}: the update kernels form the A2C / PPO gradient"
    if not one_launch_rollout:   # (asked last: a shape the rollout kernels refuse is named by what is wrong with it)
        return False, "the rollout is per tick: the update kernels go with the one-launch rollout"
    return True, ""


def admitted_shape(one_launch_rollout, n_policies, n_agents, head_sizes, fc_dims, obs_size, dtype, normalize_return,
                   normalize_advantage, neg_pos_env_ratio, world_size, algorithm):
    """(True, "") when the update kernels serve this policy, else (False, why)"""
    if n_policies != 1:
        return False, f"{n_policies} policies: the update kernels train one"
    if n_agents != 1:
        return False, f"{n_agents} agents: the update kernels train one per replica"
    heads = [int(a) for a in head_sizes]
    if len(heads) != 1:
        return False, f"{len(heads)} action heads: the update kernels take one"
    if not 1 <= heads[0] <= MAX_ACTIONS:
        return False, f"{heads[0]} actions: the update kernels take 1 to {MAX_ACTIONS}"
    return _admitted_tail(fc_dims, obs_size, OBS_SIZES, f"the update kernels exist for {list(OBS_SIZES)}", dtype,
                          normalize_return, normalize_advantage, neg_pos_env_ratio, world_size, algorithm, one_launch_rollout)


def normalize_refusal(n_envs, n_agents):
    """(True, "") when the normalising launches serve a policy of n_agents agents on n_envs replicas, else (False, why)"""
    columns = int(n_envs) * int(n_agents)
    if columns < 2:
        return False, (f"{columns} column per tick: the unbiased standard deviation of normalize_return / "
                       "normalize_advantage is NaN there")
    return True, ""


def policy_parameters(model):
    """the eight parameters of a two-hidden-layer, one-head FullyConnected in the kernels' order"""
    layers = [model.fc["0"][0], model.fc["1"][0], model.policy_head[0], model.vf_head]
    return [p for layer in layers for p in (layer.weight, layer.bias)]


class FlatPolicy:
    """`flat` [P] float32; every parameter of the module becomes a view of it (same values), so a kernel that writes `flat`
    has updated the module, and `load_state_dict` / `copy_` on the module write `flat`."""

    def __init__(self, model):
        assert len(model.fc) == 2 and len(model.policy_head) == 1, "not a network of the update kernels"
        params = policy_parameters(model)
        H, O, A = int(params[0].shape[0]), int(params[0].shape[1]), int(params[4].shape[0])
        slices = tensor_slices(H, O, A)
        assert [tuple(p.shape) for p in params] == [s for _, s in slices], "not the layout of the update kernels"
        assert [id(p) for p in params] == [id(p) for p in model.parameters()], "not the order of the module's parameters"
        self.H, self.O, self.A = H, O, A
        self.flat = torch.empty(net_floats(H, O, A), dtype=torch.float32, device=params[0].device)
        with torch.no_grad():
            for p, (at, shape) in zip(params, slices):
                view = self.flat[at:at + p.numel()].view(shape)
                view.copy_(p.detach().float())
                p.data = view
        self.params = params

    def bound(self):
        """every parameter still is the view it was made (nobody has re-assigned `.data`)"""
        return all(p.data_ptr() == self.flat.data_ptr() + 4 * at
                   for p, (at, _) in zip(self.params, tensor_slices(self.H, self.O, self.A)))


class _PgUpdateLaunches:
    """What PgUpdateKernels and PgGridworldUpdateKernels share: the geometry rules, the buffers the launches hand to each
    other and the five wrappers, written on rows = T * E * n recorded rows (n agents of the policy per replica), the P
    floats of the network, the floats of the rollout's packed policy and the Apply grid.  A class supplies its entry names,
    n, the two LDS sizes, the packed size and `_shape_args`.  Blocks and grids: the gradient kernel's block is its tile
    (TILE threads) and its grid one block per tile up to one per compute unit (the rest are grid-stride trips); the value
    kernel takes the largest block of 64 / 128 / 256 threads that still gives every compute unit one; Apply has one thread
    per float of the larger of the network and the packed policy.  `gradients_block` / `blocks_per_cu`: another gradient
    entry's block size and how many of its blocks a compute unit holds (the tile stays TILE rows)."""

    def _setup(self, function_manager, names, batch_shape, H, O, A, values_lds, gradients_lds, packed_floats, device,
               compute_units, gradients_block=TILE, blocks_per_cu=1):
        self.T, self.E = int(batch_shape[0]), int(batch_shape[1])
        self.n = int(batch_shape[2]) if len(batch_shape) == 3 else 1
        self._batch_dims = len(batch_shape)
        assert self.E >= 1 and self.T >= 1 and self.n >= 1, batch_shape
        self.H, self.O, self.A = int(H), int(O), int(A)
        self.device = torch.device(device)
        if compute_units is None:
            compute_units = torch.cuda.get_device_properties(self.device).multi_processor_count
        self.compute_units = int(compute_units)
        self.P = net_floats(H, O, A)
        self.packed_floats = int(packed_floats)
        self.names = names
        function_manager.initialize_functions(self.names)
        (self.fn_values, self.fn_returns, self.fn_gradients, self.fn_reduce,
         self.fn_apply) = (function_manager.get_function(n) for n in self.names)
        self.values_lds, self.gradients_lds = values_lds, gradients_lds
        self.gradients_block, self._blocks_per_cu = int(gradients_block), int(blocks_per_cu)
        self.apply_grid = -(-max(self.P, self.packed_floats) // APPLY_THREADS)
        # (the normalising, the down-sampling and the GAE launches: their entries and buffers come with the first
        # `normalize` / `downsample` / `gae_returns`)
        self._function_manager, self._fn_normalize, self._fn_downsample, self._fn_gae = function_manager, None, None, None
        assert max(self.values_lds, self.gradients_lds) <= LDS_LIMIT
        self.sampled = None                # (positives, negatives kept) of the last `downsample`
        self.E_recorded = self.E           # replicas of the recorded batch; `downsample` may leave self.E below it
        self._geometry(self.E)
        # ---- what the launches hand to each other, allocated once for the recorded batch; the attributes are views of
        # the first rows of these (all of them unless `downsample` kept fewer replicas)
        f32 = dict(dtype=torch.float32, device=self.device)
        self._whole = {name: torch.zeros(self.rows, **f32) for name in ("values", "returns", "advantages")}
        self._whole["partials"] = torch.zeros((self.gradients_grid, self.P + SUMS), **f32)
        self._views()
        self.grads = torch.zeros(self.P, **f32)
        self.sumsq = torch.zeros(TENSORS, **f32)
        self.sums = torch.zeros(SUMS, **f32)

    def _geometry(self, E):
        """blocks and grids of every launch for a batch of T ticks of E replicas (the class docstring's rules)"""
        self.E = int(E)
        self.rows = self.T * self.E * self.n
        block = VALUES_MAX_THREADS
        while block > 64 and -(-self.rows // block) < self.compute_units:
            block //= 2
        self.values_block = block
        self.values_grid = max(1, min(-(-self.rows // block), 8 * self.compute_units))
        self.returns_grid = -(-(self.E * self.n) // RETURNS_THREADS)
        self.tiles = -(-self.rows // TILE)
        self.gradients_grid = max(1, min(self.tiles, self.compute_units * self._blocks_per_cu))
        # (the normalising launches: one block per chunk of a tick's E * n columns)
        self.columns = self.E * self.n
        self.normalize_chunks = -(-self.columns // NORMALIZE_CHUNK)
        self.normalize_grid = self.T * self.normalize_chunks

    def _views(self):
        """the buffers of the current geometry: the first T * E * n floats of each whole one, in the batch's shape"""
        shape = (self.T, self.E) if self._batch_dims == 2 else (self.T, self.E, self.n)
        for name, whole in self._whole.items():
            if name == "partials":
                self.partials = whole[:self.gradients_grid]
            elif name == "partials_returns" or name == "partials_advantages":
                setattr(self, name, whole[:self.T * self.normalize_chunks * 2].view(self.T, self.normalize_chunks, 2))
            else:
                setattr(self, name, whole[:self.rows].view(shape))

    # ------------------------------------------------------------------------------------------------ the launches
    def _check_batch(self, t, tail, dtype=torch.float32, rows=None):
        rows = self.rows if rows is None else rows
        assert t.dtype == dtype and t.is_contiguous() and t.numel() == rows * tail, (tuple(t.shape), rows, tail)

    def _check_flat(self, *tensors, numel=None):
        for t in tensors:
            assert t.numel() == (self.P if numel is None else numel) and t.dtype == torch.float32 and t.is_contiguous()

    def _shape_args(self, per_row):
        """the shape arguments of an entry: `per_row` for Values and Gradients, else Reduce and Apply"""
        raise NotImplementedError

    def compute_values(self, obs, theta, out=None, block=None, grid=None):
        """values [T, E(, n)] = v(obs); obs [T, E, n, O]"""
        out = self.values if out is None else out
        self._check_batch(obs, self.O)
        assert obs.shape[-1] == self.O, tuple(obs.shape)
        self._check_flat(theta)
        self._check_flat(out, numel=self.rows)
        block = self.values_block if block is None else int(block)
        assert block % 64 == 0 and 64 <= block <= VALUES_MAX_THREADS
        self.fn_values(obs, theta, np.int64(self.rows), *self._shape_args(True), out, block=(block, 1, 1),
                       grid=(self.values_grid if grid is None else int(grid), 1), shared=self.values_lds)
        return out

    def discounted_returns(self, rewards, done, gamma, values=None, returns=None, advantages=None):
        """(returns, returns - values) [T, E(, n)] from the existing HipDiscountedReturns: n agents, an output row of width 1
        whose column 0 is the value; done [T, E] is the replica's"""
        values = self.values if values is None else values
        returns = self.returns if returns is None else returns
        advantages = self.advantages if advantages is None else advantages
        self._check_batch(rewards, 1)
        self._check_batch(done, 1, torch.int32, rows=self.T * self.E)
        self._check_flat(values, returns, advantages, numel=self.rows)
        self.fn_returns(rewards, done, values, np.int32(1), np.int32(0), np.float32(gamma), np.int32(self.T), np.int32(self.E),
                        np.int32(self.n), returns, advantages, block=(RETURNS_THREADS, 1, 1), grid=(self.returns_grid, 1),
                        shared=0)
        return returns, advantages

    def gae_returns(self, rewards, done, gamma, gae_lambda, values=None, returns=None, advantages=None, wavefronts=None):
        """(returns, returns - values) [T, E(, n)] with returns = A + values, A the GAE(lambda) advantages of
        losses.gae_returns, from HipPgGaeReturns in `discounted_returns`' position; done [T, E] is the replica's.  A block
        is 64 columns x `wavefronts` segments of ticks (None: `gae_wavefronts` of the current geometry)."""
        values = self.values if values is None else values
        returns = self.returns if returns is None else returns
        advantages = self.advantages if advantages is None else advantages
        self._check_batch(rewards, 1)
        self._check_batch(done, 1, torch.int32, rows=self.T * self.E)
        self._check_flat(values, returns, advantages, numel=self.rows)
        if self._fn_gae is None:
            self._function_manager.initialize_functions([GAE_ENTRY])
            self._fn_gae = self._function_manager.get_function(GAE_ENTRY)
        S = gae_wavefronts(self.columns, self.T, self.compute_units) if wavefronts is None else int(wavefronts)
        assert S in GAE_WAVEFRONTS, S
        self._fn_gae(rewards, done, values, np.float32(gamma), np.float32(gae_lambda), np.int32(self.T), np.int32(self.E),
                     np.int32(self.n), returns, advantages, block=(GAE_TILE * S, 1, 1),
                     grid=(-(-self.columns // GAE_TILE), 1), shared=8 * GAE_TILE * S if S > 1 else 0)
        return returns, advantages

    # ---------------------------------------------------------------------------------------- neg_pos_env_ratio
    def _downsample_setup(self):
        """first use: the three entries of wd_kernels_pg_select.hsaco and what they write, sized once for the recorded
        batch (a trainer without neg_pos_env_ratio pays for neither)"""
        if self._fn_downsample is not None:
            return
        self._function_manager.initialize_functions(list(DOWNSAMPLE_ENTRIES))
        self._fn_downsample = tuple(self._function_manager.get_function(n) for n in DOWNSAMPLE_ENTRIES)
        E, rows = self.E_recorded, self.T * self.E_recorded * self.n
        i32 = dict(dtype=torch.int32, device=self.device)
        self.select_blocks = -(-E // SELECT_SCAN_THREADS)
        self.positive, self.keys, self.keep_ids = (torch.zeros(E, **i32) for _ in range(3))   # (keys: uint32 bits)
        self.block_counts, self.counts = torch.zeros(self.select_blocks, **i32), torch.zeros(3, **i32)
        self._kept = {"obs": torch.zeros(rows * self.O, dtype=torch.float32, device=self.device),
                      "actions": torch.zeros(rows, **i32),
                      "rewards": torch.zeros(rows, dtype=torch.float32, device=self.device),
                      "done": torch.zeros(self.T * E, **i32)}

    def select_scan(self, done, epoch, seed_words, positive=None, keys=None, block_counts=None):
        """positive [E] = done == 2 at any tick, keys [E] = word 0 of Philox counter (e, epoch, DOWNSAMPLE_STREAM_TAG, 6)
        under `seed_words`, one positive count per block of 256 replicas; done [T, E] of the recorded batch"""
        self._downsample_setup()
        E = self.E_recorded
        self._check_batch(done, 1, torch.int32, rows=self.T * E)
        positive, keys = self.positive if positive is None else positive, self.keys if keys is None else keys
        block_counts = self.block_counts if block_counts is None else block_counts
        assert positive.numel() == keys.numel() == E and block_counts.numel() == self.select_blocks
        self._fn_downsample[0](done, np.int32(self.T), np.int32(E), np.uint32(int(epoch) & 0xFFFFFFFF),
                               np.uint32(DOWNSAMPLE_STREAM_TAG), np.uint32(int(seed_words[0]) & 0xFFFFFFFF),
                               np.uint32(int(seed_words[1]) & 0xFFFFFFFF), positive, keys, block_counts,
                               block=(SELECT_SCAN_THREADS, 1, 1), grid=(self.select_blocks, 1), shared=0)

    def select_keep(self, ratio, positive=None, keys=None, block_counts=None, keep_ids=None, counts=None):
        """keep_ids [K] ascending and counts = (K, positives, negatives kept) by losses._sample_positive_negative_env_ids'
        rule: every replica when there is no positive or pos + int(pos * ratio) >= E, else the positives and the
        int(pos * ratio) negatives with the smallest (key, replica id)"""
        self._downsample_setup()
        positive, keys = self.positive if positive is None else positive, self.keys if keys is None else keys
        block_counts = self.block_counts if block_counts is None else block_counts
        keep_ids, counts = self.keep_ids if keep_ids is None else keep_ids, self.counts if counts is None else counts
        E = self.E_recorded
        assert positive.numel() == keys.numel() == E and keep_ids.numel() >= E and counts.numel() == 3
        assert all(t.dtype == torch.int32 and t.is_contiguous() for t in (positive, keys, block_counts, keep_ids, counts))
        self._fn_downsample[1](keys, positive, block_counts, np.int32(block_counts.numel()), np.int32(E), np.float64(ratio),
                               keep_ids, counts, block=(SELECT_KEEP_THREADS, 1, 1), grid=(1, 1), shared=0)

    def gather_columns(self, K, pairs, keep_ids=None):
        """dst [T][K][w] = src [T][E][keep_ids][w] for up to four (src, dst) pairs of 4-byte elements in ONE launch; the
        width w of a pair is src's elements per (tick, replica)"""
        self._downsample_setup()
        keep_ids, E, K = self.keep_ids if keep_ids is None else keep_ids, self.E_recorded, int(K)
        assert 1 <= K <= E and keep_ids.numel() >= K and 1 <= len(pairs) <= 4
        args = []
        for src, dst in pairs:
            w = src.numel() // (self.T * E)
            assert src.numel() == self.T * E * w and dst.numel() == self.T * K * w and w >= 1, (tuple(src.shape), K)
            assert src.element_size() == dst.element_size() == 4 and src.is_contiguous() and dst.is_contiguous()
            args += [src, dst, np.int32(w)]
        args += [_NULL, _NULL, np.int32(0)] * (4 - len(pairs))
        self._fn_downsample[2](keep_ids, np.int32(K), np.int32(self.T), np.int32(E), *args, block=(GATHER_THREADS, 1, 1),
                               grid=(self.T * -(-K // GATHER_CHUNK), 1), shared=0)

    def downsample(self, done, ratio, epoch, obs, actions, rewards, seed_words=(0, 0)):
        """`trainer.neg_pos_env_ratio` before `compute_values`: scan, keep, ONE read-back of (K, positives, negatives
        kept), and -- when K < E -- the gather of the kept columns of the four batch arrays, after which every later launch
        has the geometry of a (T, K) batch and the buffers are views of the first T * K * n rows of the whole ones (no
        allocation).  Returns (obs, actions, rewards, done) as the later launches are to read them: the arguments
        themselves when every replica is kept.  `epoch`: the update's number (the keys of two updates differ)."""
        self._downsample_setup()
        if self.E != self.E_recorded:
            self._geometry(self.E_recorded)
            self._views()
        self._check_batch(obs, self.O)
        self._check_batch(actions, 1, torch.int32)
        self._check_batch(rewards, 1)
        self.select_scan(done, epoch, seed_words)
        self.select_keep(ratio)
        K, positives, negatives = self.counts.tolist()
        self.sampled = (positives, negatives)
        assert 1 <= K <= self.E_recorded and positives + negatives == K, (K, positives, negatives)
        if K == self.E_recorded:
            return obs, actions, rewards, done
        T, n = self.T, self.n
        kept = {"obs": self._kept["obs"][:T * K * n * self.O].view(T, K, n, self.O),
                "actions": self._kept["actions"][:T * K * n].view(T, K, n, 1),
                "rewards": self._kept["rewards"][:T * K * n].view(T, K, n), "done": self._kept["done"][:T * K].view(T, K)}
        self.gather_columns(K, [(obs, kept["obs"]), (actions, kept["actions"]), (rewards, kept["rewards"]), (done, kept["done"])])
        self._geometry(K)
        self._views()
        return kept["obs"], kept["actions"], kept["rewards"], kept["done"]

    def _normalize_setup(self):
        """first use: the three entries of wd_kernels_pg_norm.hsaco and what they write (a policy that never normalises
        pays for neither); partials [T][chunks][2] = (mean, M2) per chunk of a tick"""
        ok, why = normalize_refusal(self.E, self.n)
        assert ok, why
        self._function_manager.initialize_functions(list(NORMALIZE_ENTRIES))
        self._fn_normalize = tuple(self._function_manager.get_function(n) for n in NORMALIZE_ENTRIES)
        f32 = dict(dtype=torch.float32, device=self.device)
        rows, chunks = self.T * self.E_recorded * self.n, -(-self.E_recorded * self.n // NORMALIZE_CHUNK)
        for name in ("norm_returns", "norm_advantages"):
            self._whole[name] = torch.zeros(rows, **f32)
        for name in ("partials_returns", "partials_advantages"):
            self._whole[name] = torch.zeros(self.T * chunks * 2, **f32)
        self._views()

    def normalize(self, normalize_return, normalize_advantage, returns=None, values=None, advantages=None,
                  norm_returns=None, norm_advantages=None):
        """losses._normalise between `discounted_returns` and `gradients`, in A2C.compute_loss_and_metrics' order, as two
        or three launches of one block per (tick, chunk of 4096 columns):
            normalize_return:     Moments(returns), NormalizeReturns -> norm_returns, advantages = norm_returns - values
            normalize_advantage:  Moments(advantages), NormalizeAdvantages -> norm_advantages
            both:                 Moments(returns), NormalizeReturns (which also leaves the chunk moments of its
                                  advantages), NormalizeAdvantages
        Out of place but for `advantages` under normalize_return, which becomes norm_returns - values as in the framework.
        Returns (advantages, returns) as the gradient launch is to read them."""
        if not (normalize_return or normalize_advantage):
            return (self.advantages if advantages is None else advantages), (self.returns if returns is None else returns)
        if self._fn_normalize is None:
            self._normalize_setup()
        fn_moments, fn_returns, fn_advantages = self._fn_normalize
        returns, values = self.returns if returns is None else returns, self.values if values is None else values
        advantages = self.advantages if advantages is None else advantages
        norm_returns = self.norm_returns if norm_returns is None else norm_returns
        norm_advantages = self.norm_advantages if norm_advantages is None else norm_advantages
        self._check_flat(returns, values, advantages, norm_returns, norm_advantages, numel=self.rows)
        shape = (np.int32(self.T), np.int32(self.columns), np.int32(self.normalize_chunks))
        launch = dict(block=(NORMALIZE_THREADS, 1, 1), grid=(self.normalize_grid, 1), shared=0)
        eps = np.float32(NORMALIZE_EPS)
        if normalize_return:
            fn_moments(returns, *shape, self.partials_returns, **launch)
            fn_returns(returns, values, self.partials_returns, *shape, eps, norm_returns, advantages,
                       self.partials_advantages if normalize_advantage else _NULL, **launch)
        else:
            fn_moments(advantages, *shape, self.partials_advantages, **launch)
        if normalize_advantage:
            fn_advantages(advantages, self.partials_advantages, *shape, eps, norm_advantages, **launch)
        return (norm_advantages if normalize_advantage else advantages), (norm_returns if normalize_return else returns)

    def gradients(self, obs, actions, theta, ent_coeff, vf_coeff, advantages=None, returns=None, partials=None):
        """per-block partials [blocks, P + 4]: the gradient of
        mean(-logp(a) adv) + vf_coeff mean((v - ret)^2) - ent_coeff mean(entropy) over the rows, then the block's four
        sums; the grid is the number of rows of `partials`"""
        advantages = self.advantages if advantages is None else advantages
        returns = self.returns if returns is None else returns
        partials = self.partials if partials is None else partials
        self._check_batch(obs, self.O)
        assert obs.shape[-1] == self.O, tuple(obs.shape)
        self._check_batch(actions, 1, torch.int32)
        self._check_flat(advantages, returns, numel=self.rows)
        self._check_flat(theta)
        assert partials.dim() == 2 and partials.shape[1] == self.P + SUMS and partials.is_contiguous()
        assert partials.dtype == torch.float32
        self.fn_gradients(obs, actions, advantages, returns, theta, np.int64(self.rows), *self._shape_args(True),
                          np.float32(1.0 / self.rows), np.float32(ent_coeff), np.float32(vf_coeff), partials,
                          block=(self.gradients_block, 1, 1), grid=(int(partials.shape[0]), 1), shared=self.gradients_lds)
        return partials

    def reduce(self, partials=None, grads=None, sumsq=None, sums=None):
        """flat gradient [P], sums of squares per tensor [8], the four sums"""
        partials = self.partials if partials is None else partials
        grads, sumsq, sums = (self.grads if grads is None else grads, self.sumsq if sumsq is None else sumsq,
                              self.sums if sums is None else sums)
        assert partials.shape[1] == self.P + SUMS and partials.is_contiguous() and partials.dtype == torch.float32
        assert grads.numel() == self.P and sumsq.numel() == TENSORS and sums.numel() == SUMS
        self.fn_reduce(partials, np.int32(partials.shape[0]), *self._shape_args(False), grads, sumsq, sums,
                       block=(REDUCE_THREADS, 1, 1), grid=(REDUCE_BLOCKS, 1), shared=0)
        return grads, sumsq, sums

    def apply(self, theta, exp_avg, exp_avg_sq, step, lr, max_norm=None, packed=None, grads=None, sumsq=None,
              betas=(0.9, 0.999), eps=1e-8):
        """clip (max_norm None or <= 0: off), Adam step number `step` (1 for the first), and the rollout's packed policy.
        step_size = lr / (1 - beta1^step) and sqrt(1 - beta2^step) are Python floats, as in torch.optim.Adam."""
        grads, sumsq = self.grads if grads is None else grads, self.sumsq if sumsq is None else sumsq
        self._check_flat(theta, exp_avg, exp_avg_sq, grads)
        assert step >= 1 and sumsq.numel() == TENSORS
        if packed is not None:
            self._check_flat(packed, numel=self.packed_floats)
        beta1, beta2 = betas
        bc1, bc2 = 1 - beta1 ** float(step), 1 - beta2 ** float(step)
        self.fn_apply(theta, exp_avg, exp_avg_sq, grads, sumsq, _NULL if packed is None else packed, *self._shape_args(False),
                      np.float32(max_norm if max_norm else 0.0), np.float32(lr / bc1), np.float32(bc2 ** 0.5),
                      np.float32(1 - beta1), np.float32(beta2), np.float32(1 - beta2), np.float32(eps),
                      block=(APPLY_THREADS, 1, 1), grid=(self.apply_grid, 1), shared=0)

    # ------------------------------------------------------------------------------------------------ reading back
    def gradient_norm(self, sumsq=None):
        """the 2-norm of the whole gradient before clipping, from the reduce launch (reads the device)"""
        return float(torch.sqrt((self.sumsq if sumsq is None else sumsq).double().sum()))

    def metrics(self, rewards, actions, ent_coeff, vf_coeff, ppo, normalize_return=False, normalize_advantage=False):
        """the metric dict of losses.A2C.compute_loss_and_metrics_from_logits from what the launches left behind: values,
        returns, advantages and the four sums (reads the device; call after `reduce`); rewards [T, E, n], actions
        [T, E, n, 1].  After `normalize(normalize_return, normalize_advantage)` the four sums are those of the normalised
        pair the gradient launch read, the raw and the normalised means are both reported and the explained variance is
        formed from the normalised pair, as the framework does.  After `downsample` the arrays are those it returned and
        its two counts are reported under the framework's names."""
        R = float(self.rows)
        s_pg, s_ent, s_vf, s_adv = (float(v) for v in self.sums.double().tolist())
        policy_loss = -(s_adv if ppo else s_pg) / R   # PPO at ratio 1: min(ratio * A, clamp(ratio) * A) = A
        vf_loss, entropy = s_vf / R, s_ent / R
        adv, ret = self.advantages.reshape(self.T, self.E, self.n), self.returns.reshape(self.T, self.E, self.n)
        norm_adv = self.norm_advantages.reshape(adv.shape) if normalize_advantage else adv
        norm_ret = self.norm_returns.reshape(ret.shape) if normalize_return else ret
        var_explained = torch.clamp(1 - norm_adv.var() / (norm_ret.var() + 1.0e-10), min=-1.0)
        m = {
            "VF loss coefficient": vf_coeff, "Entropy coefficient": ent_coeff,
            "Total loss": float(np.float32(policy_loss + vf_coeff * vf_loss - ent_coeff * entropy)),
            "Policy loss": policy_loss, "Value function loss": vf_loss,
            "Mean rewards": rewards.mean().item(), "Max. rewards": rewards.max().item(),
            "Min. rewards": rewards.min().item(), "Mean value function": self.values.mean().item(),
            "Mean advantages": adv.mean().item(), "Mean (norm.) advantages": norm_adv.mean().item(),
            "Mean (discounted) returns": ret.mean().item(), "Mean normalized returns": norm_ret.mean().item(),
            "Mean entropy": entropy, "Variance explained by the value function": var_explained.item(),
        }
        if self.sampled is not None:   # (after `downsample`: the framework's two counts)
            m["Num of Positive Sampled Envs"], m["Num of Negative Sampled Envs"] = self.sampled
        af = actions.reshape(self.T, self.E, self.n, -1).float()
        over_agents, over_time, over_envs = (af.std(dim=d).mean(dim=(0, 1)) for d in (2, 0, 1))
        for h in range(af.shape[-1]):
            m[f"Std. of action_{h} over agents"] = over_agents[h].item()
            m[f"Std. of action_{h} over envs"] = over_envs[h].item()
            m[f"Std. of action_{h} over time"] = over_time[h].item()
        return m


class PgUpdateKernels(_PgUpdateLaunches):
    """The five launches for one (E, T, H, O, A): one agent per replica, every entry takes (H, O, A).
    gradients_entry "matrix": the third launch is HipPgGradientsMx, its block, grid, LDS bytes and partials sized for it."""

    def __init__(self, function_manager, E, T, H, O, A, device, compute_units=None, gradients_entry="lanes"):
        assert H in HIDDEN and O in OBS_SIZES and 1 <= A <= MAX_ACTIONS, (H, O, A)
        assert gradients_entry in GRADIENTS_ENTRIES, gradients_entry
        self.gradients_entry = gradients_entry
        matrix = gradients_entry == "matrix"
        self._setup(function_manager, kernel_names(H, O, gradients_entry), (T, E), H, O, A, values_lds_bytes(H, O),
                    gradients_matrix_lds_bytes(H, O) if matrix else gradients_lds_bytes(H, O), packed_floats(H, O, A), device,
                    compute_units, gradients_block=MATRIX_THREADS if matrix else TILE,
                    blocks_per_cu=MATRIX_BLOCKS_PER_CU[H] if matrix else 1)

    def _shape_args(self, per_row):
        return np.int32(self.H), np.int32(self.O), np.int32(self.A)


def log_refusal(policy, reason):
    logging.info(f"trainer.fused_update \"all\", policy '{policy}': {reason}; its update runs on the framework path")
