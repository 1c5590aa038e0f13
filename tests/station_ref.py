"""One band of real signals through the whole receiver chain: what tests/test_station_cpu.py and tests/test_gpu_station.py
share.  A plain module: no fixtures, nothing of the code under test.

  the scene       scene(): one deterministic complex ADC stream of NS = 2^23 samples, fourteen modulated carriers over a
                  noise floor, every carrier's phase from an exact 32-bit NCO word, the slow modulating waveforms made at
                  the receiver rate and interpolated linearly up to the ADC rate
  the station     the parameters of every stage for the K = 21 receivers that read it (the module's constants)
  the references  one function per stage that applies the stage's own reference (tests/*_ref.py) to the arrays its
                  predecessors wrote; reference_chain() feeds them one another's outputs, rounded to the types the device
                  hands over, and check_stages() feeds them a run's own arrays and compares
  the radio facts functions over the arrays of a run (the reference chain's or the device's): the text that was sent, the
                  tone at its frequency, the sideband on its side, the gate shut on noise

Rates are nominal: the stream is called 20 MS/s, so that M = 1024, hop 512, R = 4 give the receiver rate 9765.625 Hz of
carrier_ref and eq_ref, and Audio's 3072 / 625 gives 48 kHz.

Timing.  Tuner output i is centred on ADC sample 2048 i + 18175.5 (the prototype's 4096 taps and the low-pass's 64 rows;
only complete windows give an output, so the series starts there).  The modulating sample m is put at ADC sample
2048 m + OFFSET with OFFSET = 1792, which is tuner output m + LATE, LATE = -8 (to 0.0003 samples).  A change of tone or
key is the linear ramp between the modulating samples m and m + 1, so its middle meets the receivers' series half-way
between two samples: the matched filters of Fsk never see a window that holds as much of one tone as of the other, and
the decision margins of fsk_ref and morse_ref hold by construction and not by the noise's grace.

What the reference chain made of the scene's first draft, and what was done (all of it on the references alone):
  - CW noise.  With noise 20 dB (and 30 dB) below the carrier the samples next to an envelope's threshold crossings fall
    where the noise puts them, and morse_ref's margin does not hold for l; it holds from 40 dB on (0.0062 against
    MARGIN = 0.0028 for both receivers), so l and m carry noise 40 dB down.  The key goes down CW_LEAD = 8 samples
    into the scene: a meter whose first block of 64 holds nothing but the zeros of Blanker's delay and noise puts its
    thresholds at the noise's level, and no margin measured against the later peak survives that.
  - m's keyer has shift 1.  At 40 samples per dot the scene holds "VVV THE", seven pairs of unlike marks; from 2.5 times
    the true two-dot length a tracker of shift 2 (a quarter of the error per pair) ends 24 % off, one of shift 1 at 0.6 %,
    within test_morse_cpu.py's 8.0 %.
  - Fsk's margin.  Behind the blanker the first sample that is not zero is BLANKER_DELAY, and it is that sample which sees
    one tap of equal magnitude in both matched filters (ref_fsk says how the modules' rule is applied to it).
  - The blanker in the audio.  A blanked stretch of an AM carrier is a hole of the carrier's own level, twice the peak of
    a tone of depth 0.5: f's audio cannot stay below the tone's peak at an impulse.  fact_blanker asserts what holds: f's
    audio stays within the carrier's level there, g's exceeds twice that (the reference: 1.02 and 10 .. 14 times).
  - The whistle.  Adapt's leaky NLMS takes any steady sinusoid by its power, so a tone survives NOTCH by under 1 dB only
    where it lies well below the whistle: h's tone has depth 0.02 (14 dB below the whistle 20 dB below the carrier),
    mu / leak are set for about 9 dB on the whistle and 0.5 dB on the tone.
  - Squelch and Denoise.  A first block (frame) that holds only Blanker's zeros and RxFilter's rise gives a RELATIVE
    squelch a floor of nearly nothing, on which it opens on noise, and gives Denoise a noise estimate that takes hundreds
    of frames to rise: the squelch's block is 64 with attack 1, so that block 0 reaches into the filtered signal.
  - The mirror receiver cm (c's carrier read with upper=False) is metered and not gated, so that its audio can be
    compared with c's; the noise-only receivers and n are gated on RELATIVE thresholds.

Constants.  Every figure recorded here comes from the reference chain in float64 (tests/test_station_cpu.py measures each
again and asserts the record); none was taken from a device run."""
import functools
import time

import numpy as np

import adapt_ref as AR
import audio_ref as UR
import blanker_ref as BR
import carrier_ref as CR
import channelizer_ref as ZR
import demod_ref as DR
import denoise_ref as NR
import eq_ref as ER
import fsk_ref as FR
import mixer_ref as MR
import morse_ref as KR
import rxfilter_ref as XR
import scope_ref as PR
import squelch_ref as SR
import tuner_ref as TR

MASK = 0xFFFFFFFF
F32 = np.float32
FS = 20.0e6
CH = DR.CHAIN                                     # M = 1024, hop 512, T = 64, R = 4, four taps per branch
M, HOP, NTAPS, DECIM = CH["nchan"], CH["hop"], CH["ntaps"], CH["decim"]
UP = HOP * DECIM                                  # ADC samples per receiver sample: 2048
RATE = FS / UP                                    # 9765.625
NS = 1 << 23
OFFSET = 1792
LATE = -8                                         # modulating sample m is tuner output m + LATE
NMOD = NS // UP + 2                               # modulating samples
PROTO = TR.kaiser_prototype_wide(M, CH["proto_taps"])
LOWPASS = TR.kaiser_lowpass(NTAPS, DECIM)
NROWS = ZR.nrows_of(NS, PROTO.size, HOP)          # 16377
NRX = TR.noutputs_of(NROWS, NTAPS, DECIM)         # 4079 samples per receiver

NAMES = ["a", "b", "c", "d", "e", "f", "g", "h", "i", "j", "k", "l", "m", "n", "cm", "q0", "q1", "q2", "q3", "q4", "q5"]
K = len(NAMES)                                    # 21 = 16 + 5
RX = {name: j for j, name in enumerate(NAMES)}
NOISE_ONLY = [RX[f"q{i}"] for i in range(6)]
SILENT = NOISE_ONLY + [RX["cm"]]                  # at gain 0 in the mixer

AMP, AMP_F, NOISE = 0.035, 0.02, 0.003
SSB_BAND = (300.0, 2700.0)
TONE = dict(a=1000.0, b=800.0, e=600.0, f=500.0, h=700.0, i=1200.0, n=0.0)
DEPTH = dict(a=0.5, b=0.5, f=0.5, h=0.02, i=0.5)
SSB_TONES = dict(c=(700.0, 1900.0), d=(900.0, 1700.0))
B_OFFSET_WORDS = 1503                             # b's carrier above its tuned word: 6.9989 Hz
B_OFFSET_HZ = B_OFFSET_WORDS * FS / 2.0 ** 32
FM_TAU, FM_DEV0 = 750.0e-6, 500.0                 # de-emphasis, and the deviation a tone far below 1 / (2 pi tau) gets
WHISTLE_HZ, WHISTLE = 2200.0, 0.1                 # h: a second carrier 20 dB below the first
I_NOISE_DB = 10.0                                 # i: noise at the receiver rate 10 dB below the carrier
CW_NOISE_DB = dict(l=40.0, m=40.0)                # l, m: noise at the receiver rate 40 dB below the carrier (the module's docstring)
CW_SPD = dict(l=16, m=40)
CW_OFFSET_WORDS = dict(l=1 << 16, m=1 << 14)      # the CW carriers above their tuned words: 1 / 32 and 1 / 128 cycles per sample
SCOPE = dict(nfft=256, hop=128, avg=2)
SCOPE_BIN = dict(l=SCOPE["nfft"] // 32, a=0)
IMPULSES = [200 + 310 * q + (7 * q) % 13 for q in range(12)]     # modulating samples of f's impulses
IMPULSE_AMP = 0.3
KEYED = (NMOD // 4, 3 * NMOD // 4)                # n: the carrier is on for these modulating samples

RTTY_TEXT = "THE QUICK BROWN FOX 73"
CW_TEXT = dict(l="VVV THE QUICK", m="VVV THE")
CW_LEAD = 8                                       # modulating samples of key up before the first dot


def _word(k, r):
    return ((k << 22) + r) & MASK


CARRIER_WORDS = dict(a=_word(37, 123457), b=_word(101, -311111) + B_OFFSET_WORDS, c=_word(200, 654321), d=_word(301, -400000),
                     e=_word(511, 1500000), f=_word(640, -987654), h=_word(700, 250000), i=_word(777, -1800000),
                     j=_word(850, 999), k=_word(1023, -1900000), l=_word(444, -5) + CW_OFFSET_WORDS["l"],
                     m=_word(0, -700000) + CW_OFFSET_WORDS["m"], n=(1 << 32) - (1 << 21) + 1234)


def _hz(word):
    return word * FS / 2.0 ** 32


def _tuner_words():
    w = {name: CARRIER_WORDS[name] for name in "aefhijkn"}
    w["g"] = w["f"]
    w["b"] = CARRIER_WORDS["b"] - B_OFFSET_WORDS
    w["l"] = CARRIER_WORDS["l"] - CW_OFFSET_WORDS["l"]
    w["m"] = CARRIER_WORDS["m"] - CW_OFFSET_WORDS["m"]
    bfo = {}
    for name, carrier, upper in (("c", "c", True), ("cm", "c", False), ("d", "d", False)):
        w[name], bfo[name] = DR.ssb_words(FS, RATE, _hz(CARRIER_WORDS[carrier]), SSB_BAND[0], SSB_BAND[1], upper)
    for i, (k, r) in enumerate(((60, 77777), (150, -1234567), (512, 3), (600, 2000000), (900, -2097152), (980, 31))):
        w[f"q{i}"] = _word(k, r)
    return [w[name] & MASK for name in NAMES], bfo


WORDS, BFO = _tuner_words()
CHANNELS = sorted({TR.channel_of(M, f)[0] for f in WORDS})

# ---- the stages' parameters -------------------------------------------------------------------------------------------
BLANKER = dict(block=48, guard=3, ramp=5, beta=BR.BETA, cap=BR.CAP)
BLANKER_OFF = [RX[name] for name in "glmn"]      # g is f's twin without the blanker; a keyed carrier is no impulse
BLANKER_RX = [(16.0, 0 if j in BLANKER_OFF else BR.ON) for j in range(K)]
BLANKER_DELAY = BLANKER["guard"] + BLANKER["ramp"]

FILTER_TAPS = 63
WIDTHS = (2500.0, 1200.0, 1800.0, 3200.0)        # AM, SSB, the decoders, FM
BANK = XR.kaiser_bank(RATE, WIDTHS, FILTER_TAPS)
FILTER_DELAY = (FILTER_TAPS - 1) // 2
SEL = [dict(c=1, cm=1, d=1, j=2, k=2, l=2, m=2, e=3).get(name, 0) for name in NAMES]

CARRIER_RX = [(CR.DSB if name == "b" else CR.OFF,) + CR.loop_gains(30.0, RATE) for name in NAMES]
HILBERT = CR.hilbert(31)


def _demod_rx():
    rx = []
    for name in NAMES:
        if name in BFO:
            rx.append((DR.SSB, BFO[name], 0))
        elif name == "b":
            rx.append((DR.SSB, 0, DR.DC))
        elif name == "e":
            rx.append((DR.FM, 0, 0))
        else:
            rx.append((DR.AM, 0, DR.DC))
    return rx


DEMOD_RX = _demod_rx()
DEMOD = dict(rho=0.995, lam=0.9995, target=0.25, gmax=1.0e4)

SQUELCH = dict(block=64, attack=1, hang=2, ramp=16, up=SR.UP)
RELATIVE = [RX["n"]] + NOISE_ONLY
SQUELCH_RX = [(100.0, 30.0, SR.GATE | SR.RELATIVE) if j in RELATIVE else (1.0e-6, 3.0e-7, 0 if NAMES[j] == "cm" else SR.GATE)
              for j in range(K)]                   # the mirror receiver is metered only: its audio is what is compared

ADAPT = dict(taps=32, delay=1, eps=AR.EPS)
ADAPT_RX = [(AR.NOTCH, 0.0154, 2.0 ** -8) if name == "h" else (AR.OFF, 0.5, 0.0) for name in NAMES]

DENOISE = dict(nfft=256, hop=128)
DENOISE_RX = [(NR.NR if name == "i" else NR.OFF,) + NR.RX_DEFAULT[1:] for name in NAMES]
DENOISE_DELAY = DENOISE["nfft"]

EQ_SECTIONS = 2
DEEMPHASIS = ER.design(ER.LOWPASS1, RATE, 1.0 / (2.0 * np.pi * FM_TAU))
HIGH_CUT = ER.design(ER.LOWPASS, RATE, 3000.0)
EQ_RX = [[DEEMPHASIS] if name == "e" else [HIGH_CUT] if name in "abfghin" else [] for name in NAMES]

AUDIO = dict(L=3072, M=625, P=128, T=32)
AUDIO_RATE = RATE * AUDIO["L"] / AUDIO["M"]      # 48 kHz
AUDIO_PROTO = UR.kaiser_audio_prototype(AUDIO["P"], AUDIO["T"], 0.45)


def _pan(gain_db, pan):
    """mixer_pan restated"""
    g, t = 10.0 ** (gain_db / 20.0), (pan + 1.0) * np.pi / 4.0
    return [float(F32(g * np.cos(t))), float(F32(g * np.sin(t)))]


GAIN_DB = dict(a=12.0, b=12.0, c=10.0, d=10.0, e=-14.0, f=16.0, g=16.0, h=22.0, i=12.0, j=6.0, k=6.0, l=6.0, m=6.0, n=6.0)
GAINS = [[0.0, 0.0] if j in SILENT else _pan(GAIN_DB[name], -1.0 + 2.0 * j / 13.0) for j, name in enumerate(NAMES)]
MIX_RAMP, MIX_BLOCK, MIX_CEIL, MIX_REL = 8, 16, 0.5, 0.25
MIX_LIMIT = (MIX_BLOCK, MIX_CEIL, MIX_REL)
MIX_CHUNK = 32

SCOPE_ROWS = [RX["l"], RX["a"]]
SCOPE_WINDOW = PR.hann(SCOPE["nfft"])

FSK_W = 16
FSK_BANK = [FR.modem(RATE, RATE / FR.SPS, FR.MARK * RATE, FR.SPACE * RATE, FSK_W)]
FSK_SEL = [(0, FR.ON | (FR.REVERSE if name == "k" else 0)) if name in "jk" else (0, 0) for name in NAMES]

MORSE_W = 20
_KEYERS = {name: KR.keyer(spd * 20.0 / 1.2, 20.0, MORSE_W) for name, spd in CW_SPD.items()}
MORSE_BANK = [_KEYERS["l"], (_KEYERS["m"][0], int(2.5 * _KEYERS["m"][1])) + _KEYERS["m"][2:4] + (1,)]
MORSE_SEL = [(dict(l=0, m=1)[name], KR.ON) if name in "lm" else (0, 0) for name in NAMES]
MORSE_TWO_BOUND = {name: 0.0375 + 2.0 / (4 * spd) + 0.03 for name, spd in CW_SPD.items()}       # test_morse_cpu.py: 9.9 %, 8.0 %

# ---- recorded figures of the reference chain (float64; tests/test_station_cpu.py re-measures each) ---------------------
REF_MIRROR_DB = 74.62                             # X + 3: c's two tones against the mirror receiver's same bins
REF_NOTCH_DB = 9.00                               # Y + 3: the whistle's bin, Adapt's input against its output
REF_SINAD_GAIN_DB = 5.44                          # + 1: i's SINAD behind Denoise against in front of it
CARRIER_OFFSET_BOUND_HZ = 0.0092                  # |freq rate / 2 - true offset| of b's loop over the last quarter, the worst
MIRROR_MARGIN_DB, NOTCH_MARGIN_DB, SINAD_MARGIN_DB, LEVEL_DB = 3.0, 3.0, 1.0, 0.1

# the float32 models' worst deviation from the double references on the reference chain's own arrays, per stage, in the
# stage's own metric; TOL_STATION = 7 x that, the project's margin
MODEL_WORST_STATION = dict(channelizer=9.90e-08, tuner=3.20e-07, rxfilter=3.46e-08, carrier=1.10e-07, demod_am=1.31e-07,
                           demod_fm=6.98e-08, demod_ssb=2.93e-07, denoise=3.81e-07, audio=3.70e-08, scope=2.72e-07, fsk=5.18e-07,
                           morse=4.43e-07)
TOL_STATION = {k: 7 * v for k, v in MODEL_WORST_STATION.items()}


# ---- the scene --------------------------------------------------------------------------------------------------------

def rtty_codes():
    return FR.ita2_encode(RTTY_TEXT)


def _modulation():
    """per occupied receiver (amp float64 [NMOD], phase float64 [NMOD], add complex128 [NMOD] or None): the complex
    envelope amp exp(i phase) + add on the carrier, at the receiver rate"""
    m = np.arange(NMOD, dtype=np.float64)
    t = m / RATE
    rng = np.random.default_rng(2025)
    zero = np.zeros(NMOD)
    out = {}
    for name in "abfhi":
        out[name] = [(AMP_F if name == "f" else AMP) * (1.0 + DEPTH[name] * np.cos(2.0 * np.pi * TONE[name] * t)), zero, None]
    for name, sign in (("c", 1.0), ("d", -1.0)):
        f1, f2 = SSB_TONES[name]
        out[name] = [zero, zero, 0.5 * AMP * (np.exp(sign * 2j * np.pi * f1 * t) + np.exp(sign * 2j * np.pi * f2 * t + 1.0j))]
    dev = FM_DEV0 * abs(1.0 + 2j * np.pi * TONE["e"] * FM_TAU)
    out["e"] = [np.full(NMOD, AMP), dev / TONE["e"] * np.sin(2.0 * np.pi * TONE["e"] * t), None]
    imp = np.zeros(NMOD, np.complex128)
    imp[IMPULSES] = IMPULSE_AMP * np.exp(2j * np.pi * rng.uniform(size=len(IMPULSES)))
    out["f"][2] = imp
    out["h"][2] = WHISTLE * AMP * np.exp(2j * np.pi * WHISTLE_HZ * t)
    sigma = AMP * 10.0 ** (-I_NOISE_DB / 20.0) / np.sqrt(2.0)
    out["i"][2] = sigma * (rng.standard_normal(NMOD) + 1j * rng.standard_normal(NMOD))
    line = FR.keying(rtty_codes(), sps=FR.SPS, lead=4.0, tail=4.0)
    assert line.size < NMOD - 64, line.size
    line = np.concatenate([line, np.zeros(NMOD - line.size, bool)])
    for name, mark, space in (("j", FR.MARK, FR.SPACE), ("k", FR.SPACE, FR.MARK)):
        out[name] = [np.full(NMOD, AMP), 2.0 * np.pi * (0.25 + np.cumsum(np.where(line, space, mark))), None]
    for name, spd in CW_SPD.items():
        key = KR.keying(CW_TEXT[name], spd, CW_LEAD, 0)
        assert key.size < NMOD - 8 * spd, (name, key.size)
        key = np.concatenate([key, np.zeros(NMOD - key.size, bool)])
        db = CW_NOISE_DB[name]
        add = None
        if db is not None:
            s = AMP * 10.0 ** (-db / 20.0) / np.sqrt(2.0)
            add = s * (rng.standard_normal(NMOD) + 1j * rng.standard_normal(NMOD))
        out[name] = [AMP * key, zero, add]
    out["n"] = [AMP * ((m >= KEYED[0]) & (m < KEYED[1])), zero, None]
    return out


@functools.lru_cache(maxsize=1)
def scene():
    """-> float32 [NS, 2] for the packing (|re|, |im| < 1 asserted), made 2^19 samples at a time"""
    mod = _modulation()
    out = np.empty((NS, 2), F32)
    rng = np.random.default_rng(78)
    step = 1 << 19
    for lo in range(0, NS, step):
        i = np.arange(lo, lo + step, dtype=np.int64)
        tm = np.maximum(i - OFFSET, 0) / float(UP)
        m0 = tm.astype(np.int64)
        fr = tm - m0
        x = NOISE * (rng.standard_normal(step) + 1j * rng.standard_normal(step))
        for name, (amp, ph, add) in mod.items():
            c = amp[m0] + (amp[m0 + 1] - amp[m0]) * fr
            if ph.any():
                c = c * np.exp(1j * (ph[m0] + (ph[m0 + 1] - ph[m0]) * fr))
            if add is not None:
                c = c + (add[m0] + (add[m0 + 1] - add[m0]) * fr)
            nco = 2.0 * np.pi * ((CARRIER_WORDS[name] * i) & MASK).astype(np.float64) / 2.0 ** 32
            x += c * np.exp(1j * nco)
        assert np.abs(x.real).max() < 1.0 and np.abs(x.imag).max() < 1.0
        out[lo:lo + step, 0], out[lo:lo + step, 1] = x.real, x.imag
    out.setflags(write=False)
    return out


# ---- the stage references ---------------------------------------------------------------------------------------------

def c64(x):
    x = np.asarray(x)
    out = np.empty(x.shape, np.complex64)
    out.real, out.imag = x.real, x.imag
    return out


def ref_channelizer(x):
    """x complex [NS] (the unpacked stream) -> complex128 [rows, len(CHANNELS)], the listed channels in the list's order"""
    return ZR.channelizer_ref(np.asarray(x, np.complex128), M, HOP, PROTO)[:, CHANNELS]


def _columns():
    kr = [TR.channel_of(M, f) for f in WORDS]
    return np.array([CHANNELS.index(k) for k, _ in kr]), [r for _, r in kr]


def ref_tuner(rows):
    cols, res = _columns()
    y = np.asarray(rows)[:, cols].astype(np.complex128)
    return TR.fir_decim_mm(TR.mix(y, res, [0] * K, HOP), LOWPASS, DECIM).T


def ref_blanker(tun):
    r = BR.BlankerRef(BLANKER_RX, **BLANKER)
    return r.process(c64(tun)), r.read()


def ref_rxfilter(blk):
    return XR.rxfilter_ref(c64(blk), BANK, SEL)


def ref_carrier(flt, track=None):
    """-> (u complex128, status); track: the batch length at which the status is read along the way -> also the list of
    (samples fed, freq) of receiver b"""
    r = CR.CarrierRef(CARRIER_RX, HILBERT, **CR.PARAMS)
    z = c64(flt)
    if track is None:
        return r.process(z), r.read()
    outs, seen = [], []
    for lo in range(0, z.shape[1], track):
        outs.append(r.process(z[:, lo:lo + track]))
        seen.append((min(lo + track, z.shape[1]), float(r.v[RX["b"]])))
    return np.concatenate(outs, axis=1), r.read(), seen


def ref_demod(car):
    return DR.demod_ref(c64(car), DEMOD_RX, **DEMOD)


def ref_squelch(flt, dem):
    r = SR.SquelchRef(SQUELCH_RX, **SQUELCH)
    out, lv, st = r.process(c64(flt), np.asarray(dem, F32))
    return out, lv, st, r.read()


def ref_adapt(sql):
    out, w, _ = AR.adapt_ref(np.asarray(sql, F32), ADAPT_RX, **ADAPT)
    return out, w


def ref_denoise(adp, dtype=np.float64):
    s = NR.Stream(DENOISE["nfft"], DENOISE["hop"], NR.window(**DENOISE), DENOISE_RX, dtype=dtype)
    return s.process(np.asarray(adp, F32)), s.noise()


def ref_eq(dns):
    out, st, _ = ER.eq_ref(np.asarray(dns, F32), EQ_RX, EQ_SECTIONS)
    return out, st


def ref_audio(eq):
    return UR.audio_ref(np.asarray(eq, F32), AUDIO["L"], AUDIO["M"], AUDIO["P"], AUDIO["T"], AUDIO_PROTO)


def ref_mixer(aud, chunk=MIX_CHUNK):
    r = MR.MixerRef(GAINS, MIX_RAMP, MIX_LIMIT, chunk=chunk)
    out, pcm = r.process(np.ascontiguousarray(aud, dtype=F32))
    return out, pcm, r.read()


def ref_scope(z):
    """the lines of the two slots -> float64 [2, lines, nfft]"""
    return PR.scope_ref(np.asarray(z)[SCOPE_ROWS], SCOPE["nfft"], SCOPE["hop"], SCOPE["avg"], SCOPE_WINDOW)


def ref_fsk(flt, sel=None, f32=False):
    """-> (chars per receiver, d, margin, status).  fsk_ref's margin leaves out a receiver's first sample behind zero
    history, where one tap of equal magnitude in both filters gives pm = ps in any arithmetic.  Behind the blanker that
    sample is BLANKER_DELAY, the first that is not zero: the zeros before it are a batch of their own (s = 0, nothing
    is compared), and the rule is applied to the first sample of the rest."""
    r, z, D = FR.FskRef(FSK_BANK, FSK_SEL if sel is None else sel, FSK_W, f32=f32), c64(flt), BLANKER_DELAY
    if z.shape[1] <= D or z[:, :D].any():
        return FR.run_cuts(r, z)

    def before(i, r):
        if i == 1:
            r.first = r.on.copy()
    return FR.run_cuts(r, z, [D, z.shape[1] - D], before)


def ref_morse(flt, f32=False):
    """-> (chars per receiver, p, margin, status, peak)"""
    return KR.run_cuts(KR.MorseRef(MORSE_BANK, MORSE_SEL, MORSE_W, f32=f32, **KR.PARAMS), c64(flt))


FSK_PLAIN_SEL = [(0, FR.ON)]                       # k's row through a receiver without REVERSE


def reference_chain(x):
    """The whole chain on the unpacked stream x (complex [NS]): every stage's reference on its predecessors' outputs,
    rounded to the type the device hands over (complex64, float32) before the next stage reads them.  -> the dict of
    arrays the radio facts take, the doubles before the rounding under "<name>64", and "seconds"."""
    t0 = time.time()
    R = {}
    R["rows64"] = ref_channelizer(x)
    R["rows"] = c64(R["rows64"])
    R["tun64"] = ref_tuner(R["rows"])
    R["tun"] = c64(R["tun64"])
    R["blk"], R["blanker_status"] = ref_blanker(R["tun"])
    R["flt64"] = ref_rxfilter(R["blk"])
    R["flt"] = c64(R["flt64"])
    R["car64"], R["carrier_status"], R["carrier_track"] = ref_carrier(R["flt"], track=64)
    R["car"] = c64(R["car64"])
    R["car"][[j for j in range(K) if CARRIER_RX[j][0] == CR.OFF]] = R["flt"][[j for j in range(K) if CARRIER_RX[j][0] == CR.OFF]]
    R["dem64"] = ref_demod(R["car"])
    R["dem"] = R["dem64"].astype(F32)
    R["sql"], R["sql_levels"], R["sql_states"], R["squelch_status"] = ref_squelch(R["flt"], R["dem"])
    R["adp"], R["adapt_weights"] = ref_adapt(R["sql"])
    R["dns64"], R["denoise_noise"] = ref_denoise(R["adp"])
    R["dns"] = R["dns64"].astype(F32)
    R["eq"], R["eq_state"] = ref_eq(R["dns"])
    R["aud64"] = ref_audio(R["eq"])
    R["aud"] = R["aud64"].astype(F32)
    R["pcm"] = UR.pcm_ref(R["aud"])
    R["mix"], R["mix_pcm"], R["mixer_status"] = ref_mixer(R["aud"])
    poisoned = R["aud"].copy()
    poisoned[SILENT] = np.nan
    R["mix_nan"] = ref_mixer(poisoned)[0]
    for name in ("tun", "blk", "flt"):
        R["scope_" + name] = ref_scope(R[name])
    R["fsk_chars"], R["fsk_d"], R["fsk_margin"], R["fsk_status"] = ref_fsk(R["flt"])
    R["fsk_plain"] = ref_fsk(R["flt"][RX["k"]:RX["k"] + 1], FSK_PLAIN_SEL)[0][0]
    R["morse_chars"], R["morse_p"], R["morse_margin"], R["morse_status"], R["morse_peak"] = ref_morse(R["flt"])
    R["seconds"] = time.time() - t0
    return R


# ---- the comparisons of section 4.1 -----------------------------------------------------------------------------------

def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[x.dtype.itemsize if x.dtype.kind != "c" else 4])


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(bits(got), bits(want)), (what, np.argwhere(bits(got) != bits(want))[:4].tolist())


def _status(got, want, what):
    for name in want.dtype.names:
        assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), (what, name, got[name], want[name])


def demod_errors(got, ref):
    return {("demod_" + DR.MODE_NAMES[m].lower()): e for m, e in DR.err_by_mode(np.asarray(got), ref, DEMOD_RX).items()}


def _rel(got, ref):
    return float(np.max(np.abs(np.asarray(got, np.complex128) - ref)) / np.max(np.abs(ref)))


def stage_checks(D, x=None):
    """{stage: a function (inputs) -> the figures it measured}, each comparing the arrays of the run D with the stage's
    reference on D's own arrays of the stage's predecessors; it raises AssertionError where they differ.  `inputs` are
    the predecessors' arrays the reference is given, by default D's own."""
    tol = TOL_STATION

    def within(figures):
        for k, v in figures.items():
            assert v <= tol[k], (k, v, tol[k])
        return figures

    def channelizer(rows=None):
        return within(dict(channelizer=_rel(D["rows"], ref_channelizer(x))))

    def tuner(rows=None):
        return within(dict(tuner=_rel(D["tun"], ref_tuner(D["rows"] if rows is None else rows))))

    def blanker(z=None):
        out, st = ref_blanker(D["tun"] if z is None else z)
        _same(D["blk"], out, "blanker")
        _status(D["blanker_status"], st, "blanker")
        return {}

    def rxfilter(z=None):
        ref = ref_rxfilter(D["blk"] if z is None else z)
        return within(dict(rxfilter=float(np.abs(D["flt"].astype(np.complex128) - ref).max())))

    def carrier(z=None):
        z = D["flt"] if z is None else z
        ref, st = ref_carrier(z)
        off = [j for j in range(K) if CARRIER_RX[j][0] == CR.OFF]
        on = [j for j in range(K) if CARRIER_RX[j][0] != CR.OFF]
        _same(D["car"][off], c64(z)[off], "carrier, OFF rows")
        e = float(CR.err_rows(D["car"][on], ref[on]).max())
        got = D["carrier_status"]
        t = tol["carrier"]
        assert np.abs(CR.theta_diff(got["theta"][on], st["theta"][on])).max() <= t / (2 * np.pi) * 2.0 ** 32, "carrier theta"
        for name in ("freq", "err"):
            assert np.abs(got[name][on].astype(np.float64) - st[name][on]).max() <= t / np.pi, ("carrier", name)
        assert np.array_equal(got["locked"], st["locked"]), "carrier locked"
        return within(dict(carrier=e))

    def demod(z=None):
        return within(demod_errors(D["dem"], ref_demod(D["car"] if z is None else z)))

    def squelch(z=None, a=None):
        out, lv, st, status = ref_squelch(D["flt"] if z is None else z, D["dem"] if a is None else a)
        _same(D["sql"], out, "squelch out")
        _same(D["sql_levels"], lv, "squelch levels")
        _same(D["sql_states"], st, "squelch states")
        _status(D["squelch_status"], status, "squelch")
        return {}

    def adapt(a=None):
        out, w = ref_adapt(D["sql"] if a is None else a)
        _same(D["adp"], out, "adapt out")
        _same(D["adapt_weights"], w, "adapt weights")
        return {}

    def denoise(a=None):
        out, noise = ref_denoise(D["adp"] if a is None else a)
        e = max(NR.metric(D["dns"], out), NR.metric(D["denoise_noise"], noise))
        return within(dict(denoise=e))

    def eq(a=None):
        out, st = ref_eq(D["dns"] if a is None else a)
        _same(D["eq"], out, "eq out")
        _same(D["eq_state"], st, "eq state")
        return {}

    def audio(a=None):
        ref = ref_audio(D["eq"] if a is None else a)
        _same(D["pcm"], UR.pcm_ref(D["aud"]), "audio pcm")
        return within(dict(audio=float(np.abs(D["aud"].astype(np.float64) - ref).max())))

    def mixer(a=None):
        out, pcm, st = ref_mixer(D["aud"] if a is None else a, D.get("mix_chunk", MIX_CHUNK))
        _same(D["mix"], out, "mixer out")
        _same(D["mix_pcm"], pcm, "mixer pcm")
        _status(D["mixer_status"], st, "mixer")
        return {}

    def scope(z=None):
        e = max(PR.err(D["scope_" + name], ref_scope(D[name])) for name in ("tun", "blk", "flt"))
        return within(dict(scope=e))

    def fsk(z=None):
        chars, d, margin, st = ref_fsk(D["flt"] if z is None else z)
        e = float(np.abs(D["fsk_d"].astype(np.float64) - d).max())
        assert e <= tol["fsk"], ("fsk", e, tol["fsk"])
        for j in range(K):
            assert margin[j] >= FR.MARGIN, ("fsk margin", j, margin[j])
            got = D["fsk_chars"][j]
            for k in ("start", "code", "flags"):
                assert np.array_equal(got[k], chars[j][k]), ("fsk", j, k, got[k], chars[j][k])
            assert np.abs(got["quality"].astype(np.float64) - chars[j]["quality"]).max(initial=0.0) <= tol["fsk"], ("fsk quality", j)
            for k in ("chars", "framing", "false_starts", "state"):
                assert D["fsk_status"][k][j] == st[k][j], ("fsk", j, k)
            assert abs(float(D["fsk_status"]["d_last"][j]) - float(st["d_last"][j])) <= tol["fsk"], ("fsk d_last", j)
        return dict(fsk=e)

    def morse(z=None):
        chars, p, margin, st, peak = ref_morse(D["flt"] if z is None else z)
        scale = np.where(peak > 0, peak, 1.0)
        e = float((np.abs(D["morse_p"].astype(np.float64) - p) / scale[:, None]).max())
        assert e <= tol["morse"], ("morse", e, tol["morse"])
        for j in range(K):
            assert margin[j] >= KR.MARGIN, ("morse margin", j, margin[j])
            assert D["morse_chars"][j].tobytes() == chars[j].tobytes(), ("morse", j, D["morse_chars"][j], chars[j])
            for k in ("chars", "marks", "two", "nel", "key"):
                assert D["morse_status"][k][j] == st[k][j], ("morse", j, k)
            for k in ("pk", "fl"):
                assert abs(float(D["morse_status"][k][j]) - float(st[k][j])) <= tol["morse"] * scale[j], ("morse", j, k)
        return dict(morse=e)

    checks = dict(tuner=tuner, blanker=blanker, rxfilter=rxfilter, carrier=carrier, demod=demod, squelch=squelch, adapt=adapt,
                  denoise=denoise, eq=eq, audio=audio, mixer=mixer, scope=scope, fsk=fsk, morse=morse)
    if x is not None:
        checks = dict(channelizer=channelizer, **checks)
    return checks


def check_stages(D, x=None, only=None, inputs=None):
    """Run the comparisons (all, or the stages `only`); inputs: {stage: the keyword arguments its reference is given in
    place of D's own arrays}.  -> (figures {name: value}, failures [(stage, the assertion's text)])"""
    figures, failures = {}, []
    for stage, fn in stage_checks(D, x).items():
        if only is not None and stage not in only:
            continue
        try:
            figures.update(fn(**(inputs or {}).get(stage, {})))
        except AssertionError as e:
            failures.append((stage, str(e)[:300]))
    return figures, failures


# ---- the float32 models: MODEL_WORST_STATION ---------------------------------------------------------------------------

def model_worst(R, x):
    """the float32 models on the reference chain's arrays (each model reads what its double reference read) -> the dict
    MODEL_WORST_STATION records"""
    out = {}
    out["channelizer"] = _rel(ZR.channelizer_model_f32(x, M, HOP, PROTO)[:, CHANNELS], R["rows64"])
    cols, res = _columns()
    out["tuner"] = _rel(TR.tuner_model_f32(R["rows"][:, cols], res, [0] * K, HOP, LOWPASS, DECIM), R["tun64"])
    out["rxfilter"] = float(np.abs(XR.rxfilter_model32(R["blk"], BANK, SEL) - R["flt64"]).max())
    on = [j for j in range(K) if CARRIER_RX[j][0] != CR.OFF]
    model = CR.CarrierRef(CARRIER_RX, HILBERT, f32=True, **CR.PARAMS).process(R["flt"])
    out["carrier"] = float(CR.err_rows(model[on], R["car64"][on]).max())
    out.update(demod_errors(DR.demod_model_f32(R["car"], DEMOD_RX, **DEMOD), R["dem64"]))
    dns, noise = ref_denoise(R["adp"], np.float32)
    out["denoise"] = max(NR.metric(dns, R["dns64"]), NR.metric(noise, R["denoise_noise"]))
    out["audio"] = float(np.abs(UR.audio_model32(R["eq"], AUDIO["L"], AUDIO["M"], AUDIO["P"], AUDIO["T"], AUDIO_PROTO).astype(np.float64)
                                - R["aud64"]).max())
    out["scope"] = max(PR.err(PR.scope_model_f32(R[name][SCOPE_ROWS], SCOPE["nfft"], SCOPE["hop"], SCOPE["avg"], SCOPE_WINDOW),
                              R["scope_" + name]) for name in ("tun", "blk", "flt"))
    out["fsk"] = float(np.abs(ref_fsk(R["flt"], f32=True)[1].astype(np.float64) - R["fsk_d"]).max())
    scale = np.where(R["morse_peak"] > 0, R["morse_peak"], 1.0)
    out["morse"] = float((np.abs(ref_morse(R["flt"], f32=True)[1].astype(np.float64) - R["morse_p"]) / scale[:, None]).max())
    return out


# ---- the radio facts --------------------------------------------------------------------------------------------------

def steady(a):
    """the steady part of an audio row: its last three quarters"""
    a = np.asarray(a, np.float64)
    return a[a.size // 4:]


def spectrum(a):
    """Hann-windowed power spectrum of the steady part -> (power [N / 2 + 1], N)"""
    s = steady(a)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(s.size) / s.size)
    return np.abs(np.fft.rfft(s * w)) ** 2, s.size


def bin_of(f_hz, n, rate=AUDIO_RATE):
    return int(round(f_hz * n / rate))


def band(p, b, half=2):
    return float(p[max(b - half, 0):b + half + 1].sum())


def peaks(p, count, skip=3, guard=4):
    """the `count` largest bins away from DC, each at least `guard` bins from the ones before it"""
    p = p.copy()
    p[:skip] = 0
    out = []
    for _ in range(count):
        b = int(np.argmax(p))
        out.append(b)
        p[max(b - guard, 0):b + guard + 1] = 0
    return sorted(out)


def fact_rtty(D):
    sent = RTTY_TEXT
    for name in "jk":
        c = D["fsk_chars"][RX[name]]
        st = D["fsk_status"][RX[name]]
        assert FR.ita2_decode(c["code"], c["flags"]) == sent, (name, FR.ita2_decode(c["code"], c["flags"]))
        assert st["framing"] == 0 and st["false_starts"] == 0 and st["chars"] == len(rtty_codes()), (name, st)
    plain = D["fsk_plain"]
    assert FR.ita2_decode(plain["code"], plain["flags"]) != sent
    for j in range(K):
        if NAMES[j] not in "jk":
            assert D["fsk_chars"][j].size == 0 and D["fsk_status"]["chars"][j] == 0, j


def fact_cw(D):
    for name in "lm":
        c = D["morse_chars"][RX[name]]
        text = KR.decode(c)
        sent = CW_TEXT[name]
        assert "THE" in text and text[text.index("THE"):] == sent[sent.index("THE"):], (name, text)
        two = int(D["morse_status"]["two"][RX[name]])
        true = KR.two_of(CW_SPD[name])
        assert abs(two - true) <= MORSE_TWO_BOUND[name] * true, (name, two, true)
    for j in range(K):
        if NAMES[j] not in "lm":
            assert D["morse_chars"][j].size == 0, j


def fact_am(D):
    for name in "ab":
        p, n = spectrum(D["aud"][RX[name]])
        assert abs(peaks(p, 1)[0] - bin_of(TONE[name], n)) <= 1, (name, peaks(p, 1), bin_of(TONE[name], n))
    st = D["carrier_status"][RX["b"]]
    assert st["locked"] == 1, st
    got = float(st["freq"]) * RATE / 2.0
    assert abs(got - B_OFFSET_HZ) <= CARRIER_OFFSET_BOUND_HZ, (got, B_OFFSET_HZ, CARRIER_OFFSET_BOUND_HZ)
    return dict(offset_hz=got)


def mirror_db(D):
    p, n = spectrum(D["aud"][RX["c"]])
    q, _ = spectrum(D["aud"][RX["cm"]])
    bins = [bin_of(f, n) for f in SSB_TONES["c"]]
    return 10.0 * np.log10(sum(band(p, b) for b in bins) / sum(band(q, b) for b in bins))


def fact_ssb(D):
    for name in "cd":
        p, n = spectrum(D["aud"][RX[name]])
        want = sorted(bin_of(f, n) for f in SSB_TONES[name])
        got = peaks(p, 2)
        assert all(abs(g - w) <= 1 for g, w in zip(got, want)), (name, got, want)
    x = mirror_db(D)
    assert x >= REF_MIRROR_DB - MIRROR_MARGIN_DB, (x, REF_MIRROR_DB)
    return dict(mirror_db=x)


def tone_level_db(a, f_hz, rate):
    """the level of the tone at f_hz in the steady part of a, by projection on exp(2 pi i f t)"""
    s = steady(a)
    t = np.arange(s.size) / rate
    return 20.0 * np.log10(2.0 * abs(np.mean(s * np.exp(-2j * np.pi * f_hz * t))))


def fact_fm(D):
    j = RX["e"]
    p, n = spectrum(D["aud"][j])
    assert abs(peaks(p, 1)[0] - bin_of(TONE["e"], n)) <= 1, (peaks(p, 1), bin_of(TONE["e"], n))
    moved = tone_level_db(D["eq"][j], TONE["e"], RATE) - tone_level_db(D["dns"][j], TONE["e"], RATE)
    want = 20.0 * np.log10(abs(ER.response([DEEMPHASIS], RATE, TONE["e"])))
    assert abs(moved - want) <= LEVEL_DB, (moved, want)
    return dict(deemphasis_db=moved, predicted_db=float(want))


def impulse_positions():
    """where f's impulses arrive in the audio: (modulating sample + what the chain delays it by) x L / M"""
    late = LATE + BLANKER_DELAY + FILTER_DELAY + DENOISE_DELAY + AUDIO["T"] // 2
    return [int(round((m + late) * AUDIO["L"] / AUDIO["M"])) for m in IMPULSES]


def fact_blanker(D):
    f, g = RX["f"], RX["g"]
    st = D["blanker_status"]
    assert st["triggers"][f] >= len(IMPULSES) and st["triggers"][g] == 0, (st["triggers"][f], st["triggers"][g])
    for j in range(K):
        if j != f:
            assert st["triggers"][j] == 0 and st["blanked"][j] == 0, (j, st[j])
    # every impulse's neighbourhood holds a blanked stretch: the output is +0 there where the input was not
    blk = D["blk"]
    for m in IMPULSES:
        lo = m + LATE - 4
        assert (np.abs(blk[f, lo + BLANKER_DELAY:lo + BLANKER_DELAY + 12]) == 0).any(), m
        assert (np.abs(blk[g, lo + BLANKER_DELAY:lo + BLANKER_DELAY + 12]) > 0).all(), m
    # In the audio a blanked stretch of an AM carrier is a hole of the carrier's own level (100 % modulation, twice the
    # tone's peak at depth 0.5), whatever the impulse was: f's audio holds nothing above that level at an impulse (9 % are
    # left for the overshoot of the low-passes behind the blanker), g's holds the impulse itself, several times the carrier.
    half = 40
    for name in "fg":
        a = np.asarray(D["aud"][RX[name]], np.float64)
        carrier = 10.0 ** (tone_level_db(a, TONE["f"], AUDIO_RATE) / 20.0) / DEPTH["f"]
        for at in impulse_positions():
            if at - half < a.size // 4 or at + half >= a.size:
                continue
            top = np.abs(a[at - half:at + half]).max()
            assert (top <= 1.09 * carrier) if name == "f" else (top > 2.0 * 1.09 * carrier), (name, at, top, carrier)


def notch_db(D):
    """(the whistle's bin in Adapt's input over its output, the tone's bin likewise), dB"""
    j = RX["h"]
    n = steady(D["sql"][j]).size
    pin, pout = spectrum(D["sql"][j])[0], spectrum(D["adp"][j])[0]
    w, t = bin_of(WHISTLE_HZ, n, RATE), bin_of(TONE["h"], n, RATE)
    return 10.0 * np.log10(band(pin, w) / band(pout, w)), 10.0 * np.log10(band(pin, t) / band(pout, t))


def fact_adapt(D):
    whistle, tone = notch_db(D)
    assert whistle >= REF_NOTCH_DB - NOTCH_MARGIN_DB, (whistle, REF_NOTCH_DB)
    assert abs(tone) < 1.0, tone
    return dict(notch_db=whistle, tone_db=tone)


def sinad_db(a, f_hz, rate):
    p, n = spectrum(a)
    b = bin_of(f_hz, n, rate)
    sig = band(p, b)
    return 10.0 * np.log10(sig / (p[3:].sum() - sig))


def sinad_gain_db(D):
    j = RX["i"]
    return sinad_db(D["dns"][j], TONE["i"], RATE) - sinad_db(D["adp"][j], TONE["i"], RATE)


def fact_denoise(D):
    g = sinad_gain_db(D)
    assert g >= REF_SINAD_GAIN_DB - SINAD_MARGIN_DB, (g, REF_SINAD_GAIN_DB)
    return dict(sinad_gain_db=g)


def fact_squelch(D):
    j = RX["n"]
    st, states = D["squelch_status"], D["sql_states"]
    assert st["opens"][j] == 1, st[j]
    B = SQUELCH["block"]
    late = LATE + BLANKER_DELAY + FILTER_DELAY
    first = (KEYED[0] + late - 8) // B                 # the first block that can hold the carrier (the tuner's rise is 8 samples)
    last = (KEYED[1] + late + 8) // B
    opened = np.flatnonzero(states[j])
    assert opened.size and first + SQUELCH["attack"] - 1 <= opened[0] <= first + SQUELCH["attack"] + 1, (opened[:1], first)
    assert last + SQUELCH["hang"] - 2 <= opened[-1] <= last + SQUELCH["hang"], (opened[-1:], last)
    assert np.array_equal(opened, np.arange(opened[0], opened[-1] + 1))
    gated = bits(np.asarray(D["sql"][j], F32))
    lo, hi = int(opened[0]) * B, (int(opened[-1]) + 1) * B + SQUELCH["ramp"] + B
    assert not gated[:lo].any() and not gated[hi:].any() and gated[lo + B + SQUELCH["ramp"]:hi - 2 * B - SQUELCH["ramp"]].all()
    for q in NOISE_ONLY:
        assert st["opens"][q] == 0 and not states[q].any() and not bits(np.asarray(D["sql"][q], F32)).any(), q
        assert not bits(np.asarray(D["aud"][q], F32)).any() and not np.asarray(D["pcm"][q]).any(), q


def fact_mixer(D):
    out, aud = np.asarray(D["mix"]), np.asarray(D["aud"], np.float64)
    assert np.abs(out).max() <= F32(MIX_CEIL) and D["mixer_status"]["min_gain"].min() < 1
    assert np.array_equal(bits(D["mix_nan"]), bits(out)), "a receiver at gain 0 reached a bus"
    g = np.asarray(GAINS, F32).astype(np.float64)
    y = g.T @ aud                                                    # [Q, n]
    mag = np.abs(g).T @ np.abs(aud)
    Lb = MIX_BLOCK
    nb = y.shape[1] // Lb
    P = np.abs(y[:, :nb * Lb]).reshape(2, nb, Lb).max(axis=2)
    assert out.shape == (2, MR.outputs(Lb, 0, y.shape[1]))
    # where the limiter's gain is 1: the gain falls at once and recovers by MIX_REL of the rest per block, so it is 1
    # again (to within 2^-24) 60 blocks behind the last block over the ceiling -- the comparison leaves 64
    over = (np.maximum(P[:, :-1], P[:, 1:]) > 0.999 * MIX_CEIL)
    unity, held = np.zeros(over.shape, bool), np.full(2, 64)
    for k in range(over.shape[1]):
        held = np.where(over[:, k], 0, held + 1)
        unity[:, k] = held > 64
    assert unity.sum() > 20, unity.sum()
    worst = 0.0
    for q in range(2):
        for k in np.flatnonzero(unity[q]):
            sl = slice(k * Lb, (k + 1) * Lb)
            bound = (K + 2) * 2.0 ** -24 * mag[q, sl] + 1e-30
            d = np.abs(out[q, sl] - y[q, sl])
            assert (d <= bound).all(), (q, k, d.max(), bound.min())
            worst = max(worst, float((d / bound).max()))
    return dict(unity_blocks=int(unity.sum()), worst_of_bound=worst)


def fact_scope(D):
    for slot, name in enumerate("la"):
        tops = {src: [int(np.argmax(line)) for line in D["scope_" + src][slot]] for src in ("tun", "blk", "flt")}
        total = {src: int(np.argmax(np.asarray(D["scope_" + src][slot], np.float64).sum(axis=0))) for src in tops}
        assert total["tun"] == total["blk"] == total["flt"] == SCOPE_BIN[name], (name, total)
        if name == "a":
            assert all(t == SCOPE_BIN[name] for src in tops for t in tops[src]), tops
    return {}


FACTS = dict(rtty=fact_rtty, cw=fact_cw, am=fact_am, ssb=fact_ssb, fm=fact_fm, blanker=fact_blanker, adapt=fact_adapt,
             denoise=fact_denoise, squelch=fact_squelch, mixer=fact_mixer, scope=fact_scope)


def carrier_offset_bound(R):
    """the loop's own steady-state error: the worst |freq rate / 2 - the true offset| of b over the last quarter of the
    reference's run, read every 64 samples"""
    return max(abs(v * RATE / 2.0 - B_OFFSET_HZ) for at, v in R["carrier_track"] if at >= 3 * NRX // 4)


def controls(D):
    """the two tampered inputs of section 4.5, made on copies of the run's arrays: {stage: the inputs for check_stages}"""
    a, e = RX["a"], RX["e"]
    z = np.array(D["car"], copy=True)
    z[[a, e]] = z[[e, a]]
    return dict(demod=dict(z=z), squelch=dict(a=np.roll(np.asarray(D["dem"], F32), 1, axis=1)))
