"""A host model of one env's sliding live stream (uhc_amd/csrc/uhc_live_window.h, uhc_live.hip): which global frame sits in which slot, what a push and a
step do to len / start_ind / cur_t / base / moved / dropped, and which global frame a read of the env kernels resolves to.  Shared by
tests/test_live_window_cpu.py (which ties `discard` to the header's function, case by case) and tests/test_gpu_live_slide.py (which predicts the counters)."""


def discard(length, cap, start_ind, cur_t):
    """uhc_lw_discard, restated."""
    if length != cap or length < 1:
        return 0
    return min(max(start_ind + cur_t, 0), length - 1)


class Window:
    def __init__(self, cap, slide=True, rule=discard):
        self.cap, self.slide, self.rule = cap, slide, rule
        self.slots, self.start_ind, self.cur_t, self.base, self.moved, self.dropped, self.pushed = [], 0, 0, 0, 0, 0, 0
        self.gone = set()  # global frames slid off

    @property
    def len(self):
        return len(self.slots)

    def restart(self):
        self.slots, self.base, self.moved, self.dropped, self.pushed = [0], 0, 0, 0, 1
        self.gone = set()

    def push(self):
        """Append the stream's next frame (global index `pushed`): slide first where the rule says so; a full window drops the row."""
        if self.slide:
            s = self.rule(self.len, self.cap, self.start_ind, self.cur_t)
            assert 0 <= s <= max(self.len - 1, 0)
            if s >= 1:
                self.gone.update(self.slots[:s])
                self.slots = self.slots[s:]
                self.start_ind -= s
                self.base += s
                self.moved += len(self.slots)
        if not self.slots or self.len >= self.cap:
            self.dropped += 1
            return False
        self.slots.append(self.pushed)
        self.pushed += 1
        return True

    def reset(self):
        self.cur_t, self.start_ind = 0, 0

    def step(self):
        self.cur_t += 1

    def read(self, t):
        """The global frame the env kernels' expert_index(t, start_ind, len) resolves to."""
        i = min(self.start_ind + t, self.len - 1)
        assert 0 <= i < self.len, (i, self.len)
        g = self.slots[i]
        assert g not in self.gone and g == self.base + i
        return g


def session(cap, head=3, steps=40, ahead=4, rule=discard, slide=True):
    """head frames, reset, then one push and one step per control step.  Before and after every step, the reads t = cur_t .. cur_t + ahead of the window are
    compared with those of a stream that keeps everything: min(t, pushed - 1).  Returns the window."""
    w = Window(cap, slide=slide, rule=rule)
    w.restart()
    for _ in range(head - 1):
        assert w.push()
    w.reset()
    for _ in range(steps):
        assert w.push(), (cap, w.cur_t)
        for phase in (0, 1):
            for t in range(w.cur_t, w.cur_t + ahead + 1):
                assert w.read(t) == min(t, w.pushed - 1), (cap, w.cur_t, t)
            if phase == 0:
                w.step()
    assert w.dropped == 0 and w.base + w.len == w.pushed == head + steps
    return w
