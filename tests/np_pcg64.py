"""
Pure-Python restatement of numpy's default generator, the algorithm the device header csrc/mpk_nprng.h implements:
SeedSequence(seed) (pool size 4) -> generate_state(4, uint64) -> PCG64 seeding, the 128-bit LCG with XSL-RR output, and the three
draws the reacher resets use (next_double / uniform, the buffered next_uint32, Lemire's bounded draw behind choice([-1, 1])).
The tests hold it against np.random.default_rng before any device code is involved.
"""
M32, M64, M128 = (1 << 32) - 1, (1 << 64) - 1, (1 << 128) - 1

# numpy/random/bit_generator.pyx
INIT_A, MULT_A, INIT_B, MULT_B = 0x43B0D7E5, 0x931E8875, 0x8B51F9DD, 0x58F38DED
MIX_MULT_L, MIX_MULT_R, XSHIFT = 0xCA01F9DD, 0x4973F715, 16
POOL = 4
# PCG_DEFAULT_MULTIPLIER_128 (numpy/random/src/pcg64/pcg64.h)
PCG_MULT = (2549297995355413924 << 64) | 4865540595714422341


def entropy_words(seed: int):
    """SeedSequence's coercion of an int: 32-bit words, least significant first; 0 is one zero word"""
    assert 0 <= seed
    words = []
    while True:
        words.append(seed & M32)
        seed >>= 32
        if not seed:
            return words


def seed_sequence_state(seed: int):
    """SeedSequence(seed).generate_state(4, np.uint64) as four Python ints"""
    ent = entropy_words(seed)
    h = INIT_A

    def hashmix(v):
        nonlocal h
        v ^= h
        h = (h * MULT_A) & M32
        v = (v * h) & M32
        return v ^ (v >> XSHIFT)

    def mix(x, y):
        r = (MIX_MULT_L * x - MIX_MULT_R * y) & M32
        return r ^ (r >> XSHIFT)

    pool = [hashmix(ent[i] if i < len(ent) else 0) for i in range(POOL)]
    for s in range(POOL):
        for d in range(POOL):
            if s != d:
                pool[d] = mix(pool[d], hashmix(pool[s]))
    for s in range(POOL, len(ent)):         # never for seeds < 2^128
        for d in range(POOL):
            pool[d] = mix(pool[d], hashmix(ent[s]))
    hb = INIT_B
    w = []
    for i in range(8):
        v = pool[i % POOL] ^ hb
        hb = (hb * MULT_B) & M32
        v = (v * hb) & M32
        w.append(v ^ (v >> XSHIFT))
    return [w[2 * k] | (w[2 * k + 1] << 32) for k in range(4)]


class PCG64:
    """numpy's PCG64 with its 32-bit buffer; ``state`` is what ``bit_generator.state`` shows"""

    def __init__(self, seed: int):
        s = seed_sequence_state(seed)
        initstate, initseq = (s[0] << 64) | s[1], (s[2] << 64) | s[3]
        self.inc = ((initseq << 1) | 1) & M128
        self.s = 0
        self._step()
        self.s = (self.s + initstate) & M128
        self._step()
        self.has_uint32, self.uinteger = 0, 0

    def _step(self):
        self.s = (self.s * PCG_MULT + self.inc) & M128

    def next_uint64(self) -> int:
        self._step()
        hi, lo = self.s >> 64, self.s & M64
        x, rot = hi ^ lo, self.s >> 122
        return ((x >> rot) | (x << ((64 - rot) & 63))) & M64

    def next_uint32(self) -> int:
        if self.has_uint32:
            self.has_uint32 = 0
            return self.uinteger
        v = self.next_uint64()
        self.has_uint32, self.uinteger = 1, v >> 32
        return v & M32

    def next_double(self) -> float:
        return (self.next_uint64() >> 11) * (1.0 / 9007199254740992.0)

    def uniform(self, lo: float, hi: float) -> float:
        return lo + (hi - lo) * self.next_double()

    def bounded_uint32(self, rng: int) -> int:
        """Lemire's draw in [0, rng] on next_uint32 (numpy's buffered_bounded_lemire_uint32)"""
        excl = rng + 1
        m = self.next_uint32() * excl
        left = m & M32
        if left < excl:
            thr = (M32 - rng) % excl
            while left < thr:
                m = self.next_uint32() * excl
                left = m & M32
        return m >> 32

    def choice_pm1(self) -> int:
        """choice([-1, 1])"""
        return (-1, 1)[self.bounded_uint32(1)]

    @property
    def state(self) -> dict:
        return {"bit_generator": "PCG64", "state": {"state": self.s, "inc": self.inc},
                "has_uint32": self.has_uint32, "uinteger": self.uinteger}
