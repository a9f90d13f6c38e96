"""The guarded observation buffers of the GPU tests that hold observations to the oracle
(test_obs_instantiations.py, test_obs_shapes.py): a buffer of the engine's dtype at a chosen byte offset of a byte
tensor filled with 0x5A, with padding rows, the call that points eng.reset / eng.observe at it, and
test_obs_instantiations.py's random state pokes (test_obs_shapes.py plans its own from the view: obs_shapes.poke_plan)."""
import numpy as np

FILL, GUARD, PAD_ROWS = 0x5A, 64, 3


class Guarded(object):
    """rows x obs_shape of the engine's dtype at byte `offset` of a 0x5A-filled byte tensor."""

    def __init__(self, eng, offset):
        import torch
        self.n, self.offset = eng.N, offset
        self.ts = torch.empty((), dtype=eng.obs_dtype).element_size()
        self.blk = int(np.prod(eng.obs_shape)) * self.ts
        rows = eng.N + PAD_ROWS
        self.raw = torch.empty(offset + rows * self.blk + GUARD + 16, dtype=torch.uint8, device=eng.device)
        assert self.raw.data_ptr() % 16 == 0 and offset >= GUARD and offset % self.ts == 0
        self.fill()
        self.view = self.raw[offset:offset + rows * self.blk].view(eng.obs_dtype).view((rows,) + tuple(eng.obs_shape))
        assert self.view.data_ptr() == self.raw.data_ptr() + offset
        self.out = eng.outputs(rows=rows, obs=self.view)

    def fill(self):
        self.raw.fill_(FILL)

    def check_guards(self, what):
        end = self.offset + self.n * self.blk
        before, after = self.raw[:self.offset].cpu().numpy(), self.raw[end:].cpu().numpy()
        assert (before == FILL).all(), ("bytes before the buffer written", what, np.nonzero(before != FILL)[0][:8] - self.offset)
        assert (after == FILL).all(), ("padding rows or bytes after the buffer written", what, np.nonzero(after != FILL)[0][:8])

    def obs(self):
        return self.view[:self.n].cpu().numpy()

    def untouched(self):
        return bool((self.raw == FILL).all())


def _into(eng, call, g, mask=None):
    """eng.reset / eng.observe into g's buffer."""
    own = eng.obs
    eng.obs = g.view
    try:
        call(mask)
    finally:
        eng.obs = own
    eng.torch.cuda.synchronize()


def _poke(eng, refs, rng, obstacles):
    """Dead bodies (some under map obstacles), damaged and cleaned-up obstacles, one obstacle in agent 0's window
    (where there is one) far below the int16 range: the same pokes through zs_set_state and the oracle."""
    for e, o in enumerate(refs):
        st = eng.get_state(e)
        W, cells, O = st.W, st.W * st.H, st.O
        dw = st.dead_words.view(np.uint32)  # writes through to the record
        dead = [int(c) for c in rng.choice(cells, size=min(cells // 2, (3, 40, 300)[e % 3]), replace=False)]
        dead += [obstacles[i][1] * W + obstacles[i][0] for i in rng.choice(O, size=3, replace=False)]
        for c in dead:
            dw[c >> 5] |= np.uint32(1 << (c & 31))
            o.poke_dead(c % W, c // W)
        ax, ay = int(st.ent[0][2]), int(st.ent[0][3])
        here = [i for i in range(1, O) if st.obst_present[i]]  # still in the world (a cleaned-up one stays out)
        near = [i for i in here if abs(obstacles[i][0] - ax) <= 10 and abs(obstacles[i][1] - ay) <= 10]
        low = near[len(near) // 2] if near else here[0]
        for i in rng.choice(np.arange(1, O), size=min(O - 1, 12), replace=False):
            if i == low:
                continue
            st.obst_life[i] = int(rng.integers(-32000, 199))
            o.poke_obstacle(int(i), int(st.obst_life[i]))
            if st.obst_life[i] <= 0 and rng.integers(2):
                st.obst_present[i] = 0
                o.poke_obstacle_gone(int(i))
        st.obst_life[low] = -40000
        o.poke_obstacle(low, -40000)
        eng.set_state(e, st)
