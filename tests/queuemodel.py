"""A restatement of the megakernel's work queue in exact integers -- test infrastructure only.

What the queue promises: a launch of `num_batches` (frame, traced tile, sample) batches of 64 pixel-samples is walked as
`total_items = perm_rows * perm_cols * 64` LOGICAL items; wavefronts claim `chunk_items` of them per atomic add on a 32-bit cursor; every
logical item is decoded to a pixel-sample or found to be padding.  Every real pixel-sample must be handed out exactly once, whatever the
order of the claims, and every wavefront must find the queue dry after finitely many claims without a cursor ever passing 2^32 - 1.

The model is written from that description.  Python integers do not wrap, so every place where the device computes in 32 bits is a place
where the model can say what the exact value is -- and the tests compare (tests/test_queue_model.py)."""
import numpy as np

U32 = 1 << 32


# ---- the magic division -----------------------------------------------------------------------------------------------------------------

def magic_of(d):
    """floor(2^32 / d) as the host passes it; 2^32 does not fit 32 bits, so d = 1 gets 0xFFFFFFFF (one too small: the correction covers it)."""
    assert 1 <= d < U32
    return (U32 // d) if d > 1 else U32 - 1


def divmod_magic(n, d, magic=None):
    """(n // d, n % d) the device's way: a multiply-high estimate that is never too large, then ONE correction step.  Every intermediate
    is reduced to 32 bits as the device's registers would."""
    magic = magic_of(d) if magic is None else magic
    q = (n * magic) >> 32
    r = (n - q * d) % U32
    if r >= d:
        r = (r - d) % U32
        q = (q + 1) % U32
    return q, r


def divmod_magic_np(n, d):
    """The same over an array of uint64 values below 2^32."""
    n = np.asarray(n, np.uint64)
    q = (n * np.uint64(magic_of(d))) >> np.uint64(32)
    r = (n - q * np.uint64(d)) & np.uint64(U32 - 1)
    fix = r >= np.uint64(d)
    return q + fix.astype(np.uint64), np.where(fix, r - np.uint64(d), r)


# ---- item decoding ----------------------------------------------------------------------------------------------------------------------

class Launch:
    """The numbers a launch hands the kernel: the plan's (a dict as raytracer-public_amd.debug_launch_plan_tuned returns it) and the frame's."""

    def __init__(self, plan, num_batches, trace_bpf, spp=1, tiles_x=1, width=8, height=8, trace_slots=None):
        self.rows, self.cols = plan["perm_rows"], plan["perm_cols"]
        self.total, self.chunk, self.span = plan["total_items"], plan["chunk_items"], plan["xcd_span"]
        self.num_batches, self.trace_bpf, self.spp, self.tiles_x = num_batches, trace_bpf, spp, tiles_x
        self.width, self.height = width, height
        self.trace_slots = trace_slots          # traced-tile slot -> tile (None: the identity)


def decode(L, logical):
    """One logical item -> None (padding, or a pixel outside the frame) or (frame, tile slot, sample, p, px, py).
    64 consecutive logical items are one batch; logical batch lb sits in COLUMN lb // rows and ROW lb % rows of the transposition, and the
    batch it stands for is row * cols + column: walking lb upwards goes down a column, i.e. through batches that are `cols` apart."""
    lb, p = logical >> 6, logical & 63
    pcol, prow = divmod_magic(lb, L.rows)
    q = prow * L.cols + pcol
    if q >= L.num_batches:
        return None
    frame, qq = divmod_magic(q, L.trace_bpf)
    tslot, s = divmod_magic(qq, L.spp)
    tile = L.trace_slots[tslot] if L.trace_slots is not None else tslot
    ty, tx = divmod_magic(tile, L.tiles_x)
    px, py = tx * 8 + (p & 7), ty * 8 + (p >> 3)
    if px >= L.width or py >= L.height:
        return None
    return frame, tslot, s, p, px, py


def decode_batches(L, first, last):
    """The batch index q behind every logical batch in [first, last) (the validity rule is `q < num_batches`), vectorised."""
    lb = np.arange(first, last, dtype=np.uint64)
    pcol, prow = divmod_magic_np(lb, L.rows)
    return prow * np.uint64(L.cols) + pcol


# ---- the queue --------------------------------------------------------------------------------------------------------------------------

def ranges(L):
    """The item ranges with a cursor of their own, in exact integers: one, or eight of `span` items each (the last ones may be empty)."""
    if L.span == 0:
        return [(0, L.total)]
    return [(qi * L.span, max(qi * L.span, min(qi * L.span + L.span, L.total))) for qi in range(8)]


class Queue:
    """Cursors and wavefronts.  `claim(w)` is one call of the kernel's claim: a (first, last) item range, or None when wavefront w has found the
    queue dry (after that it must not be asked again).  Every atomic add is counted: `probes[k]` adds of `chunk` went to cursor k."""

    def __init__(self, L, xcd_of_wave):
        self.L, self.rng = L, ranges(L)
        self.xcd = list(xcd_of_wave)
        self.hop = [0] * len(self.xcd)
        self.dry = [False] * len(self.xcd)
        self.probes = [0] * len(self.rng)

    def cursor(self, k):
        return self.probes[k] * self.L.chunk

    def claim(self, w):
        assert not self.dry[w]
        L = self.L
        if L.span == 0:
            start = self.cursor(0); self.probes[0] += 1
            if start >= L.total:
                self.dry[w] = True
                return None
            return start, min(start + L.chunk, L.total)
        while True:
            k = (self.xcd[w] + self.hop[w]) & 7
            lo, hi = self.rng[k]
            start = self.cursor(k); self.probes[k] += 1          # relative to the range's first item
            if start < hi - lo:
                return lo + start, min(lo + start + L.chunk, hi)
            self.hop[w] += 1
            if self.hop[w] == 8:
                self.dry[w] = True
                return None


def drain(L, xcd_of_wave, rng):
    """Runs the queue to the end with the wavefronts' claims interleaved by `rng` (random.Random).  Returns (claimed ranges, Queue)."""
    Q = Queue(L, xcd_of_wave)
    live = list(range(len(Q.xcd)))
    got = []
    while live:
        i = rng.randrange(len(live))
        c = Q.claim(live[i])
        if c is None:
            live[i] = live[-1]; live.pop()
        else:
            got.append(c)
    return got, Q


def final_cursors(L, waves):
    """The largest value every cursor ends on with `waves` wavefronts, from a count of the adds: each range is probed once per chunk it holds,
    and once more by EVERY wavefront -- the probe that finds it dry (the `+ 1` per wavefront: a wavefront that has been told `dry` moves on and
    never probes that cursor again)."""
    out = []
    for lo, hi in ranges(L):
        chunks = -(-(hi - lo) // L.chunk)
        out.append((chunks + waves * 1) * L.chunk)
    return out
