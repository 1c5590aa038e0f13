"""The radiofax decoder's reference (include/perseus_ddc.h, "fax"): numpy in double, vectorised over a batch's samples, and
the same operation sequence in float32 (FaxRef(..., dtype=np.float32): the model).  The reference project holds no
arithmetic for this, so this file is the oracle.  A plain module: no fixtures, nothing of the code under test.

Tolerance.  f is an arctangent of a product of two filter outputs: float32 against double differs by the filter's
rounding, amplified by 1 / |y|, and by atan2f's few units in the last place.  TOL_FAX is 7 x the float32 model's worst
|f_model - f_ref| on the GPU parity test's own inputs, case(W, 9) for every window of WINDOWS and case(W, 1024) for those of
BIG_WINDOWS, every receiver and sample (tests/test_fax_cpu.py measures it into MODEL_WORST and asserts the figures); the
7 is the margin every decoder here uses.  Never taken from k_fax.  The model's atan2 is numpy's float32 one, the device's
is its own: both are good to a few units in the last place of a value below 1, 1e-7, far inside 6 x the model's worst.
The parity inputs keep the reference's |f| at or below F_MOST = 0.9, so no value sits on the arctangent's seam, where the
two arithmetics could differ by 2.

Integers.  The clock never depends on the data: npix, counts and every record's start are pure functions of inc and m and
are compared exactly.  A pixel is the rounding of g = scale v + bias; an error of TOL_FAX in every f under the boxcar is
one of at most TOL_FAX in v and |scale| TOL_FAX in g, so the device's pixel must lie between the roundings of g -+ |scale|
TOL_FAX.  Crossings, white, flags, run and the integer status follow from the pixels by the integer rule alone:
lines_from_pixels, in plain Python, is applied to the device's own pixels."""
import numpy as np

ON, REVERSE, RESTART = 0x1, 0x2, 0x4
START, STOP, ACTIVE = 0x1, 0x2, 0x4
LINE = np.dtype([("start", np.uint64), ("crossings", np.uint16), ("white", np.uint16), ("flags", np.uint16), ("run", np.uint16)])
STATUS = np.dtype([("lines", np.uint32), ("pixels", np.uint32), ("images", np.uint32), ("active", np.uint32), ("acc", np.uint32),
                   ("col", np.uint32), ("f_last", np.float64)])
INT_STATUS = ("lines", "pixels", "images", "active", "acc", "col")
BACK = 16
WINDOWS = (1, 2, 16, 255, 256)
BIG_WINDOWS = (16, 255, 256)
F_MOST = 0.9
# worst |f_model - f_ref| per window over case(W, 9) and, for BIG_WINDOWS, case(W, 1024): test_fax_cpu.py measures and asserts
MODEL_WORST = {1: 6.42e-08, 2: 6.12e-08, 16: 1.54e-07, 255: 6.27e-07, 256: 5.97e-07}       # rounded up
TOL_FAX = 7 * max(MODEL_WORST.values())
PARITY_N = 4096
PARITY_FD = 0.2                                                            # f of white, -f of black
PARITY_NOISE = 0.1                                                         # 20 dB below the carrier


def fresh_line():
    return dict(col=0, start=0, crossings=0, white=0, level=0, run=0, cls=0, active=0, lines=0, pixels=0, images=0)


def restart_line(l, level_too):
    for k in ("col", "start", "crossings", "white", "run", "cls", "active"):
        l[k] = 0
    if level_too:
        l["level"] = 0


def lines_from_pixels(pixels, strobes, modem, state=None):
    """step 5 of the definition, pixel by pixel in plain Python: `pixels` and the sample index of each one's strobe, the
    modem's (.., width, .., start_lo, start_hi, stop_lo, stop_hi, need); `state` a fresh_line() carried from call to call
    -> (the LINE records, state)"""
    width, (s_lo, s_hi, p_lo, p_hi, need) = int(modem[2]), [int(v) for v in modem[6:11]]
    l = fresh_line() if state is None else state
    out = []
    for p, m in zip(np.asarray(pixels).tolist(), np.asarray(strobes).tolist()):
        l["pixels"] = (l["pixels"] + 1) & 0xFFFFFFFF
        if l["col"] == 0:
            l["start"] = m
        if p >= 192 and not l["level"]:
            l["level"] = 1
            l["crossings"] += 1
        if p < 64:
            l["level"] = 0
        if p >= 128:
            l["white"] += 1
        l["col"] += 1
        if l["col"] < width:
            continue
        c = l["crossings"]
        cls = START if s_lo <= c <= s_hi else STOP if p_lo <= c <= p_hi else 0
        l["run"] = 0 if not cls else 1 if cls != l["cls"] else min(l["run"] + 1, 65535)
        l["cls"] = cls
        if cls == START and l["run"] == need:
            l["active"] = 1
            l["images"] += 1
        if cls == STOP and l["run"] == need:
            l["active"] = 0
        out.append((l["start"], c, l["white"], cls | (ACTIVE if l["active"] else 0), l["run"]))
        l["lines"] += 1
        l["col"] = l["crossings"] = l["white"] = 0
    return np.array(out, dtype=LINE), l


def max_pixels(bank, n):
    """the bound of pddc_fax_max_pixels in Python's own integers"""
    inc = max(int(b[1]) for b in bank)
    return ((n * inc - 1) >> 32) + 1 if n else 0


def max_lines(bank, n):
    p, width = max_pixels(bank, n), min(int(b[2]) for b in bank)
    return (p - 1) // width + 1 if p else 0


class FaxRef:
    """the definition for (bank, sel, W) in `dtype` arithmetic: np.float64 is the reference, np.float32 the model (each
    fmaf one rounding: the product is exact in double)"""

    def __init__(self, bank, sel, W, dtype=np.float64):
        self.bank, self.W, self.dt = [tuple(b) for b in bank], int(W), np.dtype(dtype).type
        self.cdt = np.complex64 if self.dt is np.float32 else np.complex128
        self.sel = [list(s) for s in sel]
        self.reset()

    def _fresh(self):
        return dict(hist=np.zeros(self.W - 1, self.cdt), y=self.cdt(0), f=np.zeros(BACK, self.dt), acc=0, line=fresh_line())

    def reset(self):
        self.m = 0
        self.rx = [self._fresh() for _ in self.sel]
        for s in self.sel:
            s[1] &= ON | REVERSE

    def set_rx(self, j, modem, flags):
        s, r = self.sel[j], self.rx[j]
        if flags & RESTART or (not s[1] & ON and flags & ON):
            line = r["line"]
            self.rx[j] = self._fresh()
            self.rx[j]["line"] = line
            restart_line(line, True)
        if modem != s[0]:
            restart_line(r["line"], False)
        self.sel[j] = [modem, flags & (ON | REVERSE)]

    def _fma(self, a, b, c):
        if self.dt is np.float32:
            return (np.float64(a) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
        return a * b + c

    def process(self, z):
        """one batch z [nrx, n] -> (pix, lines, disc [nrx, n] of this arithmetic (0 for an OFF receiver), g, strobes): per
        receiver its pixels, LINE records, the unrounded grey values and the sample index m of every strobe"""
        z = np.asarray(z)
        nrx, n = z.shape
        dt, H = self.dt, self.W - 1
        pix, lines, gs, where = [], [], [], []
        disc = np.zeros((nrx, n), dt)
        with np.errstate(all="ignore"):
            for j in range(nrx):
                (b, flags), r = self.sel[j], self.rx[j]
                if not flags & ON or n == 0:
                    pix.append(np.zeros(0, np.uint8)); lines.append(np.zeros(0, LINE)); gs.append(np.zeros(0, dt)); where.append(np.zeros(0, np.int64))
                    continue
                h, inc, width, box, scale, bias = self.bank[b][:6]
                h = np.asarray(h, np.float32)
                x = np.concatenate([r["hist"], z[j].astype(self.cdt)])
                if dt is np.float32:
                    yr, yi = np.zeros(n, np.float32), np.zeros(n, np.float32)
                    for t in range(self.W):
                        seg = x[H - t:H - t + n]
                        yr, yi = self._fma(h[t], seg.real, yr), self._fma(h[t], seg.imag, yi)
                elif np.isfinite(x.view(np.float64)).all():
                    y = np.convolve(x, h.astype(np.float64))[H:H + n]
                    yr, yi = y.real.copy(), y.imag.copy()
                else:                                                  # 0 times infinity is NaN for every tap, as the definition has it
                    yr, yi = np.zeros(n), np.zeros(n)
                    for t in range(self.W):
                        seg = x[H - t:H - t + n]
                        yr, yi = yr + np.float64(h[t]) * seg.real, yi + np.float64(h[t]) * seg.imag
                pr_, pi_ = np.concatenate([[dt(r["y"].real)], yr[:-1]]), np.concatenate([[dt(r["y"].imag)], yi[:-1]])
                pr = yr * pr_ + yi * pi_
                pi = yi * pr_ - yr * pi_
                q = (pr - pr) + (pi - pi)
                inv_pi = np.float32(0.318309886183790672) if dt is np.float32 else 1.0 / np.pi
                d = np.where((pr == 0) & (pi == 0), dt(0), np.arctan2(pi, pr) * inv_pi + q).astype(dt)
                f = -d if flags & REVERSE else d
                disc[j] = f
                acc = r["acc"]
                carries = (np.uint64(acc) + np.arange(n + 1, dtype=np.uint64) * np.uint64(inc)) >> np.uint64(32)
                idx = np.flatnonzero(carries[1:] != carries[:-1])
                fe = np.concatenate([r["f"], f])
                first = BACK + idx - (box - 1)
                v = fe[first]
                for k in range(1, box):
                    v = v + fe[first + k]
                v = v * (dt(1) / dt(box))
                g = self._fma(dt(scale), v, dt(bias))
                p = np.where(g > 0, np.rint(np.minimum(g, 255)), 0).astype(np.uint8)
                rec, _ = lines_from_pixels(p, self.m + idx, self.bank[b], r["line"])
                pix.append(p); lines.append(rec); gs.append(g); where.append(self.m + idx)
                r["hist"] = x[x.size - H:] if H else r["hist"]
                r["y"] = self.cdt(complex(yr[-1], yi[-1]))
                r["f"] = fe[-BACK:]
                r["acc"] = (acc + n * inc) & 0xFFFFFFFF
        self.m += n
        return pix, lines, disc, gs, where

    def read(self):
        st = np.zeros(len(self.rx), STATUS)
        for j, r in enumerate(self.rx):
            l = r["line"]
            st[j] = (l["lines"], l["pixels"], l["images"], l["active"], r["acc"], l["col"], r["f"][-1])
        return st


def run_cuts(ref, z, cuts=None, before=None):
    """all of z through `ref` in the given batches -> (pix, lines, disc, g, strobes, status), each list joined per receiver"""
    nrx = z.shape[0]
    parts = [[[] for _ in range(nrx)] for _ in range(4)]
    discs, off = [], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, ref)
        out = ref.process(z[:, off:off + b])
        for k, o in zip(range(4), (out[0], out[1], out[3], out[4])):
            for j in range(nrx):
                parts[k][j].append(o[j])
        discs.append(out[2])
        off += b
    assert off == z.shape[1]
    join = lambda k: [np.concatenate(q) for q in parts[k]]
    return join(0), join(1), np.concatenate(discs, axis=1), join(2), join(3), ref.read()


# ---- the parity case -------------------------------------------------------------------------------------------------

def parity_taps(W, b):
    """a low-pass whose weight lies on its first taps (0.5^t, 24 of them, rippled by the modem's index), so that a series
    that begins behind zeros never has a filter output near zero, with small taps of either sign in the whole window"""
    t = np.arange(W, dtype=np.float64)
    h = np.where(t < 24, 0.5 ** t, 0.0) * (1.0 + 0.1 * np.cos(b + t)) + 1e-3 * np.random.default_rng(500 + b).standard_normal(W)
    return (h / h.sum()).astype(np.float32)


def bank16(W):
    """16 modems: widths 64 and 100 in turn, 2.5 .. 4 samples per pixel with odd increments (no power of two), modem 15 at
    inc = 2^31; boxcars of 1, 3 and 16; a start tone of 8 and a stop tone of 12 crossings a line, need = 2; black at f =
    -PARITY_FD, white at +PARITY_FD"""
    bank = []
    for b in range(16):
        width = 64 if b % 2 == 0 else 100
        spp = 2.5 + (1.5 if width == 64 else 0.7) * (b // 2) / 7.0
        inc = 1 << 31 if b == 15 else int(round(2.0 ** 32 / spp)) | 1
        bank.append((parity_taps(W, b), inc, width, (1, 3, 16)[b % 3], 127.5 / PARITY_FD, 127.5, 7, 9, 10, 14, 2))
    return bank


def tone_line(width, cycles):
    return np.where((np.arange(width) * cycles / width) % 1.0 < 0.5, 255, 0).astype(np.uint8)


def parity_pixels(j, width, count):
    """receiver j's picture as the sender's pixel stream: a lead of 3 + j mod 11 black pixels, then over and over three
    lines of the start tone (8 periods), one phasing line, four lines of a grey wedge with bars, three of the stop tone (12
    periods) and one black line"""
    col = np.arange(width)
    wedge = ((col * 255) // (width - 1)).astype(np.uint8)
    bars = ((col * 8 // width) * 255 // 7).astype(np.uint8)
    phasing = np.where(col < max(width // 20, 1), 255, 0).astype(np.uint8)
    frame = [tone_line(width, 8)] * 3 + [phasing, wedge, bars, wedge[::-1], bars] + [tone_line(width, 12)] * 3 + [np.zeros(width, np.uint8)]
    px = np.concatenate([np.zeros(3 + j % 11, np.uint8)] + frame * (count // (len(frame) * width) + 2))
    return px[:count]


def modulate(pixels, inc, fd, n):
    """n samples of a continuous-phase FM carrier whose frequency is (pixel / 255 - 1 / 2) 2 fd half-cycles per sample,
    the pixel of sample m being floor(m inc / 2^32)"""
    at = ((np.arange(n, dtype=np.uint64) * np.uint64(inc)) >> np.uint64(32)).astype(np.int64)
    f = (pixels[at].astype(np.float64) / 255.0 - 0.5) * 2.0 * fd
    return np.exp(1j * np.pi * np.cumsum(f))


def parity_row(j, modem, seed, reverse=False, n=PARITY_N, noise=PARITY_NOISE):
    """receiver j's series for `modem`: parity_pixels modulated at the modem's own inc, mirrored for a REVERSE receiver,
    noise 20 dB below the carrier"""
    inc, width = int(modem[1]), int(modem[2])
    z = modulate(parity_pixels(j, width, ((n * inc) >> 32) + 2), inc, PARITY_FD, n)
    if reverse:
        z = np.conj(z)
    g = np.random.default_rng(seed)
    z = z + noise * np.sqrt(0.5) * (g.standard_normal(n) + 1j * g.standard_normal(n))
    return z.astype(np.complex64)


def sel16(nrx):
    return [(j % 16, ON | (REVERSE if j % 5 == 4 else 0)) for j in range(nrx)]


_INPUTS = {}


def parity_inputs(W, nrx):
    """the rows of sel16's receivers (they do not depend on the window: a row is made with its modem's inc and width)"""
    key = 1024 if nrx == 1024 else 9
    if key not in _INPUTS:
        bank, sel = bank16(W), sel16(key)
        _INPUTS[key] = np.stack([parity_row(j, bank[b], 70000 + j, bool(fl & REVERSE)) for j, (b, fl) in enumerate(sel)])
    return _INPUTS[key][:nrx]


def case(W, nrx):
    """The parity case of window W for nrx receivers -> (bank, sel, z): bank16(W), receiver j on modem j mod 16, every
    fifth REVERSE on a mirrored signal, PARITY_N samples; 1, 5 and 9 receivers are the first rows of one array"""
    return bank16(W), sel16(nrx), parity_inputs(W, nrx)


def cut_lists(n, TT, strobe, line_end):
    """batches of 0 and 1 and odd ones; batches that end on and beside the kernel's tile seams; forty batches of one
    sample and the rest; cuts just before, on and behind a strobe and a line's last pixel (a cut "on" a sample ends a
    batch with it)"""
    def rest(c):
        assert sum(c) < n and min(c) >= 0, c
        return c + [n - sum(c)]
    assert TT < strobe < n - 2 and TT < line_end < n - 2
    return [rest([0, 1, 0, 1, 5, 0, 13, 1, 300]),
            rest([TT - 1, 1, 1, TT, TT + 1, 2 * TT - 1, 1]),
            rest([1] * 40),
            rest([strobe, 1, 1, 0, 7]),
            rest([line_end, 1, 1, 0, 7])]


def events(bank, sel1, W, z1):
    """of one fresh receiver's series: the sample of a strobe in the third tile and the sample of a line's last pixel
    behind it"""
    ref = FaxRef(bank, sel1, W)
    where = ref.process(z1)[4][0]
    width = int(bank[sel1[0][0]][2])
    k = int(np.searchsorted(where, 600))
    e = ((k // width) + 2) * width - 1
    return int(where[k]), int(where[e])


def pixel_bounds(g, scale, tol=None):
    """the least and the greatest pixel an arithmetic within TOL_FAX of the reference's f may give for the reference's g"""
    e = abs(float(scale)) * (TOL_FAX if tol is None else tol)
    with np.errstate(all="ignore"):
        lo = np.where(g - e > 0, np.rint(np.minimum(g - e, 255)), 0)
        hi = np.where(g + e > 0, np.rint(np.minimum(g + e, 255)), 0)
    return lo.astype(np.int64), hi.astype(np.int64)


def grey_bars(rows, width, levels=8):
    """the test picture: `levels` vertical bars from black to white"""
    col = np.arange(width)
    return np.tile(((col * levels // width) * 255 // (levels - 1)).astype(np.uint8), (rows, 1))


def far_from_edges(width, keep_off, levels=8):
    """the columns whose centre lies more than keep_off columns from every bar's edge (the line's two ends are edges too:
    the line before ends white)"""
    col = np.arange(width) + 0.5
    edges = np.array([-(-k * width // levels) for k in range(levels + 1)], np.float64)
    return np.abs(col[:, None] - edges[None, :]).min(axis=1) > keep_off


# ---- end to end: fax_encode -> a decoder -> fax_image ------------------------------------------------------------------

E2E_W = 32
E2E_RATE = 9765.625
E2E_LPM = 60.0 * E2E_RATE / (3.0 * 64)                                     # width 64 at 3 samples per pixel: the compressed mode
# the worst error, in grey levels, of a pixel more than box + 2 columns from a bar's edge over 20 seeds on the reference
# (test_fax_cpu.py measures and asserts it): the compressed mode's and the real one's; the bound is twice that
E2E_WORST = {False: 17.0, True: 22.0}
E2E_BOUND = 2.0 * E2E_WORST[False]


def e2e_modem(pkg, real=False, W=None):
    """the compressed mode (width 64, 3 samples per pixel, tones of 4 and 7 periods a line, 16 and 9 pixels as the real mode's 12 and 8, need 2, the deviation in the
    real mode's proportion to the pixel rate, no boxcar: a bar is 8 pixels), or the real one: 120
    lines a minute, IOC 576 at 9765.625 Hz, fax_modem's defaults"""
    if real:
        return pkg.fax_modem(E2E_RATE, 64 if W is None else W)
    return pkg.fax_modem(E2E_RATE, E2E_W if W is None else W, lpm=E2E_LPM, width=64, start_hz=4 * E2E_LPM / 60.0, stop_hz=7 * E2E_LPM / 60.0,
                         need=2, deviation_hz=400.0 * E2E_LPM / 120.0 * 64 / 1810, box=1)


def e2e_case(pkg, seed, real=False, rows=48, lead=11, noise=PARITY_NOISE):
    """-> (modem, rate, z complex64 [n], the picture sent, lead): eight grey bars behind start tone and phasing, `lead` black
    pixels ahead, noise 20 dB below the carrier"""
    modem = e2e_modem(pkg, real)
    img = grey_bars(rows, modem[2])
    dev = 400.0 if real else 400.0 * E2E_LPM / 120.0 * 64 / 1810
    z = pkg.fax_encode(img, modem, E2E_RATE, start_lines=5, phasing_lines=6, stop_lines=5, lead=lead, deviation_hz=dev)
    g = np.random.default_rng(seed)
    z = z + noise * np.sqrt(0.5) * (g.standard_normal(z.size) + 1j * g.standard_normal(z.size))
    return modem, E2E_RATE, z.astype(np.complex64), img, lead


def e2e_error(pkg, lines, pixels, modem, img, lead):
    """fax_image of one receiver's records and pixels against the picture sent: one image, all rows or one less, its column
    within 2 of where the sender's lines begin in the receiver's: `lead` pixels in, and later by the receiver's own delay,
    half the window, half the boxcar and the discriminator's half sample; -> (the worst error of the pixels more than
    box + 2 columns from a bar's edge, the column found, the rows found)"""
    width, box, W = int(modem[2]), int(modem[3]), len(modem[0])
    found = pkg.fax_image(lines, pixels, width)
    assert len(found) == 1, len(found)
    pic, col, nph = found[0]
    delay = (0.5 * (W - 1) + 0.5 * (box - 1) + 0.5) * int(modem[1]) / 2.0 ** 32
    off = (col - lead - delay + width / 2) % width - width / 2
    assert abs(off) <= 2 and nph >= 3, (col, lead, delay, nph)
    assert pic.shape[1] == width and img.shape[0] - 1 <= pic.shape[0] <= img.shape[0], pic.shape
    far = far_from_edges(width, box + 2)
    assert far.sum() >= 2 * 8
    err = np.abs(pic[:, far].astype(np.int64) - img[:pic.shape[0], far].astype(np.int64))
    return float(err.max()), col, pic.shape[0]


def model_disc(bank, sel, W, z):
    """f of every sample of a fresh receiver set in the float32 operation sequence, the rows of one modem side by side
    (FaxRef(.., np.float32) gives the same bits row by row: test_fax_cpu.py compares them on the small sets)"""
    z = np.asarray(z, np.complex64)
    nrx, n = z.shape
    H = W - 1
    out = np.zeros((nrx, n), np.float32)
    f64 = np.float64
    with np.errstate(all="ignore"):
        for b in sorted({s[0] for s in sel}):
            rows = [j for j, s in enumerate(sel) if s[0] == b and s[1] & ON]
            h = np.asarray(bank[b][0], np.float32)
            x = np.concatenate([np.zeros((len(rows), H), np.complex64), z[rows]], axis=1)
            xr, xi = x.real.astype(f64), x.imag.astype(f64)
            yr, yi = np.zeros((len(rows), n), np.float32), np.zeros((len(rows), n), np.float32)
            for t in range(W):
                yr = (f64(h[t]) * xr[:, H - t:H - t + n] + yr).astype(np.float32)
                yi = (f64(h[t]) * xi[:, H - t:H - t + n] + yi).astype(np.float32)
            zero = np.zeros((len(rows), 1), np.float32)
            pr_, pi_ = np.concatenate([zero, yr[:, :-1]], axis=1), np.concatenate([zero, yi[:, :-1]], axis=1)
            pr, pi = yr * pr_ + yi * pi_, yi * pr_ - yr * pi_
            q = (pr - pr) + (pi - pi)
            d = np.where((pr == 0) & (pi == 0), np.float32(0), np.arctan2(pi, pr) * np.float32(0.318309886183790672) + q).astype(np.float32)
            rev = np.array([bool(sel[j][1] & REVERSE) for j in rows])[:, None]
            out[rows] = np.where(rev, -d, d)
    return out
