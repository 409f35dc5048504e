"""The draw of a custom environment's fused tick (include/wd_env_tick.h), restated in numpy: agent row `row` at epoch
`e` makes ONE Philox4x32-10 call with counter (row, e, stream tag, 5) and key (seed word 0, seed word 1); head h takes
word h of the block, u = ((bits >> 8) + 1) * 2^-24; its action is the number of float32 running prefix sums of its
probability row that are < u, clamped to the last action."""
import numpy as np

from oracle.core_np import philox4x32_10, seed_words

COUNTER_WORD3 = 5
MAX_HEADS = 4


def tick_bits(rows, epochs, seed_lo, seed_hi, stream_tag):
    """the four 32-bit words of the block of every (row, epoch): uint32 [..., 4]"""
    words = philox4x32_10(np.asarray(rows, dtype=np.uint32), np.asarray(epochs, dtype=np.uint32),
                          np.uint32(int(stream_tag) & 0xFFFFFFFF), np.uint32(COUNTER_WORD3), seed_lo, seed_hi)
    return np.stack([np.asarray(w, dtype=np.uint32) for w in words], axis=-1)


def uniform_of(bits):
    """uint32 -> float32 in (0, 1]: the upper 24 bits + 1, times 2^-24 (both steps exact in float32)"""
    return ((np.asarray(bits, dtype=np.uint32) >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)


def pick(probabilities, u):
    """rows of float32 probabilities [..., A], u [...] -> int32 [...]: how many running float32 prefix sums (added in
    index order, one rounding per addition) are < u, clamped to A - 1"""
    p = np.asarray(probabilities, dtype=np.float32)
    cum = np.zeros(p.shape[:-1], dtype=np.float32)
    cnt = np.zeros(p.shape[:-1], dtype=np.int64)
    for i in range(p.shape[-1]):
        cum = p[..., i] if i == 0 else (cum + p[..., i]).astype(np.float32)
        cnt += cum < np.asarray(u, dtype=np.float32)
    return np.minimum(cnt, p.shape[-1] - 1).astype(np.int32)


class TickDraws:
    """the actions a fused tick draws, tick after tick, for every row of [n_envs, n_agents]: the epochs start at 0 (what
    `init_random` leaves) and every row advances by one per tick"""

    def __init__(self, seed, n_envs, n_agents, stream_tag):
        self.seed_lo, self.seed_hi = seed_words(seed)
        self.shape = (int(n_envs), int(n_agents))
        self.rows = np.arange(n_envs * n_agents, dtype=np.uint32)
        self.epochs = np.zeros(n_envs * n_agents, dtype=np.uint32)
        self.stream_tag = int(stream_tag)

    def draw(self, probabilities):
        """probabilities: one float32 array [n_envs, n_agents, A_h] per head -> int32 actions [n_envs, n_agents, H]"""
        assert 1 <= len(probabilities) <= MAX_HEADS
        bits = tick_bits(self.rows, self.epochs, self.seed_lo, self.seed_hi, self.stream_tag)
        self.epochs = self.epochs + np.uint32(1)
        heads = [pick(np.asarray(p).reshape(len(self.rows), -1), uniform_of(bits[:, h]))
                 for h, p in enumerate(probabilities)]
        return np.stack(heads, axis=-1).reshape(self.shape + (len(probabilities),))

    def header(self, n_rows=None):
        """the four header words of the RNG state"""
        return [self.seed_lo, self.seed_hi, len(self.rows) if n_rows is None else n_rows, 0]
