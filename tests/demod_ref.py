"""The demodulator's reference: numpy, DESIGN.md 8 / include/perseus_ddc.h "demod" restated.  `demod_ref` evaluates the
definition in double, `demod_model_f32` the same operation order in float32 (the phasor from the exact word in double,
rounded once; fmaf as one rounding of the exact double sum).  Never the code under test.

The GPU tolerances.  tests/test_demod_cpu.py::test_float32_model_against_double measures the float32 model against the
double reference on the tuner reference's outputs rounded to complex64 (2^19 LCG samples, seed 12345, M = 1024, hop 512,
T = 64, R = 4, the 1024 receivers of the tuner's parity test, 239 outputs each; rho 0.995, lambda 0.999, target 0.25,
gmax 100), per mode the worst of the four flag sets, err = max |out - ref| / max |ref| (FM: the difference modulo 2):
    AM   plain 6.63e-08  DC 2.63e-07  AGC 1.064e-06  DC+AGC 1.040e-06
    FM   plain 1.23e-07  DC 6.25e-07  AGC 6.331e-06  DC+AGC 6.331e-06
    SSB  plain 8.45e-08  DC 3.98e-07  AGC 7.66e-07   DC+AGC 1.041e-06
(the AGC divides by the envelope: max |ref| is the target, and where the envelope is still small -- FM's first outputs --
the gain is large) and ::test_float32_chain_model_against_double the chain channelizer_model_f32 -> tuner_model_f32 ->
demod_model_f32 against the three double references on chain_signal(mode), the worst of plain, DC and DC+AGC:
    AM 6.326e-07 (plain 3.79e-07)   FM 1.100e-06 (plain 8.03e-07)   SSB 3.464e-07 (plain 3.00e-07)
TOL = 7 x the worst case of each, the margin the tuner's tests use: it covers a device atan2f / sqrtf a few ulp off numpy's.  Never taken from k_demod."""
import numpy as np

MASK = 0xFFFFFFFF
AM, FM, SSB = 0, 1, 2
DC, AGC = 1, 2
MODES = (AM, FM, SSB)
MODE_NAMES = {AM: "AM", FM: "FM", SSB: "SSB"}
FLAG_SETS = (0, DC, AGC, DC | AGC)
PARAMS = dict(rho=0.995, lam=0.999, target=0.25, gmax=100.0)

MODEL_WORST_DEMOD = {AM: 1.064e-06, FM: 6.331e-06, SSB: 1.041e-06}
MODEL_WORST_DEMOD_CHAIN = {AM: 6.326e-07, FM: 1.100e-06, SSB: 3.464e-07}
TOL_DEMOD = {k: 7 * v for k, v in MODEL_WORST_DEMOD.items()}
TOL_DEMOD_CHAIN = {k: 7 * v for k, v in MODEL_WORST_DEMOD_CHAIN.items()}

# the end-to-end case: M = 1024, hop 512, T = 64, R = 4 on a nominal 80 MS/s stream -> 39 062.5 outputs per second
FS = 80.0e6
CHAIN = dict(nchan=1024, hop=512, ntaps=64, decim=4, proto_taps=4)
OUT_RATE = FS / CHAIN["hop"] / CHAIN["decim"]
CARRIER_WORD = (300 << 22) + 123457
CARRIER_HZ = CARRIER_WORD * FS / 2.0 ** 32
TONE_HZ, AM_DEPTH, FM_DEV_HZ, SSB_TONE_HZ, SSB_BAND = 1000.0, 0.5, 3000.0, 700.0, (300.0, 2700.0)


def ssb_words(fs, out_rate, carrier_hz, lo_hz, hi_hz, upper=True):
    """demod_ssb_words restated: the tuner's word in the middle of the sideband, the BFO word that moves it back"""
    mid = 0.5 * (lo_hz + hi_hz)
    sign = 1.0 if upper else -1.0
    return (int((carrier_hz + sign * mid) / fs * 4294967296.0) & MASK,
            int(round(-sign * mid / out_rate * 4294967296.0)) & MASK)


class DemodRef:
    """The streaming definition: batches of [K, n] complex values, set_rx between them.  f32 False: double (params are
    the float32 values the device gets).  f32 True: the float32 model."""

    def __init__(self, rx, rho, lam, target, gmax, f32=False):
        self.ft, self.ct = (np.float32, np.complex64) if f32 else (np.float64, np.complex128)
        self.f32 = f32
        self.rho, self.lam, self.target, self.gmax = (self.ft(np.float32(v)) for v in (rho, lam, target, gmax))
        self.invpi = np.float32(1.0 / np.pi) if f32 else 1.0 / np.pi
        self.K = len(rx)
        self.mode = np.array([r[0] for r in rx], np.int64)
        self.beta = np.array([int(r[1]) & MASK for r in rx], np.uint64)
        self.flags = np.array([r[2] for r in rx], np.int64)
        self.reset()

    def reset(self):
        K = self.K
        self.m = 0
        self.psi = np.zeros(K, np.uint64)
        self.fresh = np.ones(K, bool)
        self.zp = np.zeros(K, self.ct)
        self.dp, self.yp, self.ep = np.zeros(K, self.ft), np.zeros(K, self.ft), np.zeros(K, self.ft)

    def set_rx(self, j, mode, bfo=0, flags=0):
        bfo = int(bfo) & MASK
        if mode != self.mode[j] or flags != self.flags[j]:
            self.mode[j], self.flags[j], self.beta[j], self.psi[j] = mode, flags, bfo, 0
            self.fresh[j] = True
            self.zp[j] = 0
            self.dp[j] = self.yp[j] = self.ep[j] = 0
        else:
            self.psi[j] = (int(self.psi[j]) + (int(self.beta[j]) - bfo) * (self.m & MASK)) & MASK
            self.beta[j] = bfo

    def _fma(self, a, b, c):
        if not self.f32:
            return a * b + c
        return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)

    def process(self, z):
        ft = self.ft
        z = np.asarray(z).astype(self.ct).reshape(self.K, -1)
        n = z.shape[1]
        out = np.zeros((self.K, n), ft)
        self.e = np.zeros((self.K, n), ft)
        if n == 0:
            return out
        zprev = np.concatenate([self.zp[:, None], z[:, :-1]], axis=1)
        re, im, pre, pim = (np.ascontiguousarray(v, dtype=ft) for v in (z.real, z.imag, zprev.real, zprev.imag))
        d = np.zeros((self.K, n), ft)
        am, fm, ssb = self.mode == AM, self.mode == FM, self.mode == SSB
        ms = (np.uint64(self.m & MASK) + np.arange(n, dtype=np.uint64)) & np.uint64(MASK)
        th = (self.beta[ssb, None] * ms[None, :] + self.psi[ssb, None]) & np.uint64(MASK)
        ph = np.exp(-2j * np.pi * th.astype(np.float64) / 2.0 ** 32).astype(self.ct)
        c, s = np.ascontiguousarray(ph.real, dtype=ft), np.ascontiguousarray(ph.imag, dtype=ft)
        # non-finite samples are data like any other (include/perseus_ddc.h, "Non-finite samples"): no warnings
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            d[am] = np.sqrt(re[am] * re[am] + im[am] * im[am])
            pr = re[fm] * pre[fm] + im[fm] * pim[fm]
            pi = im[fm] * pre[fm] - re[fm] * pim[fm]
            d[fm] = np.arctan2(pi, pr) * self.invpi
            d[fm & self.fresh, 0] = 0
            d[ssb] = re[ssb] * c - im[ssb] * s
        dc, agc = (self.flags & DC) != 0, (self.flags & AGC) != 0
        dp, yp, ep = self.dp, self.yp, self.ep
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            for i in range(n):
                di = d[:, i]
                y = np.where(dc, self._fma(self.rho, yp, di - dp), di).astype(ft)
                # fmaxf / fminf, as the header spells them: a NaN operand is dropped, not passed on
                e = np.fmax(np.abs(y), self.lam * ep).astype(ft)
                g = np.fmin(self.gmax, self.target / e).astype(ft)
                out[:, i] = np.where(agc, y * g, y)
                self.e[:, i] = e
                dp, yp, ep = di, y, e
        self.dp, self.yp, self.ep = dp.copy(), yp, ep
        self.zp = z[:, -1].copy()
        self.fresh[:] = False
        self.m += n
        return out


def demod_ref(z, rx, rho, lam, target, gmax, cuts=None):
    """z [K, n] -> double [K, n], in the given batches (default: one)"""
    r = DemodRef(rx, rho, lam, target, gmax)
    return run_cuts(r, np.asarray(z), cuts)


def demod_model_f32(z64, rx, rho, lam, target, gmax):
    """the INDEPENDENT float32 model of the same operation order: complex64 [K, n] -> float32 [K, n]"""
    return DemodRef(rx, rho, lam, target, gmax, f32=True).process(np.asarray(z64, np.complex64))


def run_cuts(r, z, cuts=None):
    outs, off = [], 0
    for b in cuts or [z.shape[1]]:
        outs.append(r.process(z[:, off:off + b]))
        off += b
    assert off == z.shape[1]
    return np.concatenate(outs, axis=1)


def err(out, ref, wrap=False):
    """max |out - ref| / max |ref|; wrap (FM): the difference modulo 2, +1 and -1 are the same angle"""
    d = np.asarray(out, np.float64) - ref
    if wrap:
        d = (d + 1.0) % 2.0 - 1.0
    return float(np.max(np.abs(d)) / np.max(np.abs(ref)))


def err_by_mode(out, ref, rx):
    """{mode: err over the receivers of that mode}"""
    modes = np.array([r[0] for r in rx])
    return {m: err(out[modes == m], ref[modes == m], wrap=(m == FM)) for m in MODES if np.any(modes == m)}


def interleaved_rx(K, seed=7):
    """modes and flag sets interleaved receiver by receiver: receiver j has mode j mod 3 and flag set (j // 3) mod 4; the
    BFO words seeded random"""
    rng = np.random.default_rng(seed + K)
    words = rng.integers(0, 1 << 32, K, dtype=np.uint64)
    return [(MODES[j % 3], int(words[j]), FLAG_SETS[(j // 3) % 4]) for j in range(K)]


def chain_signal(mode, ns=1 << 19, amp=0.45, noise=0.003, seed=31):
    """The end-to-end input of one mode: a strong carrier at CARRIER_HZ (channel 300 of 1024) on a nominal 80 MS/s
    stream -- AM: a 1 kHz tone at depth 0.5; FM: a 1 kHz tone at 3 kHz deviation; SSB: a tone 700 Hz above the (absent)
    carrier -- plus a little seeded noise.  -> float32 [ns, 2] for pack24_f32"""
    n = np.arange(ns, dtype=np.int64)
    t = n.astype(np.float64) / FS
    ph = 2.0 * np.pi * ((CARRIER_WORD * n) & MASK).astype(np.float64) / 2.0 ** 32
    if mode == AM:
        x = amp * (1.0 + AM_DEPTH * np.cos(2.0 * np.pi * TONE_HZ * t)) * np.exp(1j * ph)
    elif mode == FM:
        x = amp * np.exp(1j * (ph + FM_DEV_HZ / TONE_HZ * np.sin(2.0 * np.pi * TONE_HZ * t)))
    else:
        x = amp * np.exp(1j * (ph + 2.0 * np.pi * SSB_TONE_HZ * t))
    rng = np.random.default_rng(seed + mode)
    x = x + noise * (rng.standard_normal(ns) + 1j * rng.standard_normal(ns))
    return np.stack([x.real, x.imag], axis=1).astype(np.float32)


def chain_receivers(mode):
    """(tuner words, demod rx) of the end-to-end case: the mode plain, with DC block, with DC block and AGC"""
    if mode == SSB:
        word, bfo = ssb_words(FS, OUT_RATE, CARRIER_HZ, SSB_BAND[0], SSB_BAND[1], True)
    else:
        word, bfo = CARRIER_WORD, 0
    return [word] * 3, [(mode, bfo, 0), (mode, bfo, DC), (mode, bfo, DC | AGC)]
