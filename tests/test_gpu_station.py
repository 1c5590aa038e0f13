"""The whole receiver chain on the GPU, on one band of real signals (tests/station_ref.py): packed 24-bit ADC bytes ->
Channelizer (list mode) -> Tuner -> Blanker -> RxFilter -> Carrier -> Demod -> Squelch -> Adapt -> Denoise -> Eq -> Audio
(float32 + int16) -> Mixer (two buses, limiter), with Scope on the Tuner's, Blanker's and RxFilter's rows and Fsk and Morse
on RxFilter's rows.  Every stage writes into one arena whose rows lie further apart than the longest batch and whose
padding holds nonfinite.never_read; every stage is handed its predecessor's view.

  4.1  every stage against its own reference applied to the DOWNLOADED output of its predecessors
  4.2  the same scene cut at a ragged list of ADC batches: every array and every status byte for byte
  4.3  the radio facts of tests/test_station_cpu.py on the device's arrays, with the same constants
  4.4  the arena's padding, spare rows and the gaps between blocks still hold the fill (of Fsk's and Morse's chars: what lies
       beyond max_chars -- the header promises nothing about the records between counts and that bound)
  4.5  two controls on copies of the downloaded arrays: the harness reports the stage that was tampered with"""
import types

import numpy as np
import pytest

import nonfinite as NF
import station_ref as S

pytestmark = pytest.mark.gpu
K = S.K
NA = S.UR.outputs(S.AUDIO["L"], S.AUDIO["M"], 0, S.NRX)
NM = S.MR.outputs(S.MIX_BLOCK, 0, NA)
NLINES = S.PR.nlines_of(S.NRX, S.SCOPE["nfft"], S.SCOPE["hop"], S.SCOPE["avg"])
NBLOCKS = S.NRX // S.SQUELCH["block"]
# ADC samples per batch (multiples of 8, the channelizer's rule): nothing | less than a hop: no row | ten rows: no tuner
# output | 27 outputs per receiver, fewer than any stage's history | one output | eight samples: no row | up to the
# middle of l's first dash (modulating sample 130) | up to the middle of an RTTY character (modulating sample 714) | a
# ragged one | the long rest
ENDS = [0, 256, 8704, 90624, 92672, 92680, 130 * S.UP + S.OFFSET, 714 * S.UP, 714 * S.UP + 8 * 12345, S.NS]
CUTS = [b - a for a, b in zip([0] + ENDS[:-1], ENDS)]


class Arena:
    """one device buffer filled with never_read; take() carves blocks out of it and remembers what a stage may write"""

    def __init__(self, dev, nbytes):
        import torch
        self.pattern = NF.never_read((nbytes,), np.uint8)
        self.t = torch.from_numpy(self.pattern.copy()).to(dev)
        self.off, self.blocks = 0, []

    def take(self, shape, dtype):
        import torch
        item = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape)) * item
        off = self.off = (self.off + 255) // 256 * 256 + 256               # a gap of fill between any two blocks
        assert off + n <= self.t.numel(), "arena too small"
        b = types.SimpleNamespace(t=self.t[off:off + n].view(dtype).view(shape), off=off, n=n,
                                  item=item * int(np.prod(shape[2:])), written=np.zeros(shape[:2], bool))
        self.off += n
        self.blocks.append(b)
        return b

    def intact(self):
        """every byte outside what the stages were due to write still holds the fill"""
        host = self.t.cpu().numpy()
        may = np.zeros(host.size, bool)
        for b in self.blocks:
            may[b.off:b.off + b.n] = np.repeat(b.written.reshape(-1), b.item)
        bad = np.flatnonzero((host != self.pattern) & ~may)
        return bad[:8].tolist()


def records(dtype, chars, counts):
    c = chars.cpu().numpy().view(dtype)[..., 0]
    k = counts.cpu().numpy()
    assert (k >= 0).all() and (k <= c.shape[1]).all()
    return [c[j, :k[j]].copy() for j in range(c.shape[0])]


class Station:
    """fresh objects of every stage, and the arena they write into"""

    def __init__(self, pkg, dev, longest):
        import torch
        self.pkg, self.dev = pkg, dev
        ch = self.ch = pkg.Channelizer(S.M, S.PROTO, S.HOP)
        listed = pkg.tuner_channel_list(S.M, S.WORDS)
        assert listed.tolist() == S.CHANNELS
        ch.set_channels(listed)
        self.tuner = pkg.Tuner(ch, S.WORDS, S.LOWPASS, S.DECIM)
        self.blanker = pkg.Blanker(S.BLANKER_RX, **S.BLANKER)
        assert self.blanker.delay == S.BLANKER_DELAY
        self.rxfilter = pkg.RxFilter(S.BANK, S.SEL)
        self.carrier = pkg.Carrier(S.CARRIER_RX, S.HILBERT, **S.CR.PARAMS)
        self.demod = pkg.Demod(S.DEMOD_RX, **S.DEMOD)
        self.squelch = pkg.Squelch(S.SQUELCH_RX, **S.SQUELCH)
        self.adapt = pkg.Adapt(S.ADAPT_RX, **S.ADAPT)
        self.denoise = pkg.Denoise(S.DENOISE_RX, window=S.NR.window(**S.DENOISE), **S.DENOISE)
        assert pkg.denoise_delay(S.DENOISE["nfft"]) == S.DENOISE_DELAY
        self.eq = pkg.Eq(S.EQ_RX, S.EQ_SECTIONS)
        self.audio = pkg.Audio(K, S.AUDIO["L"], S.AUDIO["M"], phases=S.AUDIO["P"], taps=S.AUDIO["T"], proto=S.AUDIO_PROTO)
        self.mixer = pkg.Mixer(S.GAINS, S.MIX_RAMP, limit=S.MIX_LIMIT)
        self.scopes = {name: pkg.Scope(K, S.SCOPE_ROWS, window=S.SCOPE_WINDOW, **S.SCOPE) for name in ("tun", "blk", "flt")}
        self.fsk = pkg.Fsk(S.FSK_BANK, S.FSK_SEL, S.FSK_W)
        self.morse = pkg.Morse(S.MORSE_BANK, S.MORSE_SEL, S.MORSE_W, **S.KR.PARAMS)
        # capacities of the longest batch, from the closed forms; every row stride is larger
        rows = longest // S.HOP + 1                                           # a batch in mid-stream completes a row per hop
        assert rows >= pkg.channelizer_rows(S.M, S.HOP, S.PROTO.size, 0, longest)
        n = rows // S.DECIM + 1
        na = pkg.audio_outputs(S.AUDIO["L"], S.AUDIO["M"], 0, n) + 1
        nm = na + S.MIX_BLOCK
        lines = n // (S.SCOPE["hop"] * S.SCOPE["avg"]) + 2
        self.cap = dict(rows=rows, n=n, na=na, nm=nm, lines=lines, blocks=n // S.SQUELCH["block"] + 1,
                        fsk=self.fsk.max_chars(n), morse=max(self.morse.max_chars(n), 1))
        c64, f32, i16, i32, u8 = torch.complex64, torch.float32, torch.int16, torch.int32, torch.uint8
        C = len(S.CHANNELS)
        shapes = dict(rows=((rows + 3, C), c64), tun=((K + 1, n + 37), c64), blk=((K + 1, n + 41), c64), flt=((K + 1, n + 43), c64),
                      car=((K + 1, n + 47), c64), dem=((K + 1, n + 53), f32), sql=((K + 1, n + 59), f32),
                      sql_levels=((K + 1, self.cap["blocks"] + 5), f32), sql_states=((K + 1, self.cap["blocks"] + 5), u8),
                      adp=((K + 1, n + 61), f32), dns=((K + 1, n + 67), f32), eq=((K + 1, n + 71), f32),
                      aud=((K + 1, na + 29), f32), pcm=((K + 1, na + 31), i16), mix=((3, nm + 23), f32), mix_pcm=((nm + 5, 2), i16),
                      scope_tun=((2, lines + 2, S.SCOPE["nfft"]), f32), scope_blk=((2, lines + 2, S.SCOPE["nfft"]), f32),
                      scope_flt=((2, lines + 2, S.SCOPE["nfft"]), f32),
                      fsk_chars=((K + 1, self.cap["fsk"] + 3, 4), i32), fsk_counts=((1, K), i32), fsk_d=((K + 1, n + 73), f32),
                      morse_chars=((K + 1, self.cap["morse"] + 3, 4), i32), morse_counts=((1, K), i32), morse_p=((K + 1, n + 79), f32))
        total = sum(int(np.prod(s)) * torch.empty((), dtype=d).element_size() + 1024 for s, d in shapes.values())
        self.arena = Arena(dev, total)
        self.b = {name: self.arena.take(s, d) for name, (s, d) in shapes.items()}
        self.parts = {name: [] for name in shapes if not name.endswith("_counts")}
        self.parts["fsk_chars"], self.parts["morse_chars"] = [[] for _ in range(K)], [[] for _ in range(K)]
        self.seen = dict(ns=0, rows=0, n=0, na=0)

    def keep(self, name, view, axis=1):
        """download a stage's view of this batch; note what it was due to write"""
        b = self.b[name]
        if axis == 1:
            b.written[:view.shape[0], :view.shape[1]] = True
        else:
            b.written[:view.shape[0], :] = True
        self.parts[name].append(view.cpu().numpy().copy())
        self.live.append((name, view, self.parts[name][-1]))
        return view

    def batch(self, packed):
        """one ADC batch through every stage, every count from the public count functions, every view handed on as it is"""
        pkg, b, cap = self.pkg, self.b, self.cap
        self.live = []
        ns = packed.numel() // 6
        due = self.ch.next_rows(ns)
        assert due == pkg.channelizer_rows(S.M, S.HOP, S.PROTO.size, self.seen["ns"], ns)
        rows = self.keep("rows", self.ch.process(packed, out=b["rows"].t[:cap["rows"]]), axis=0)
        assert rows.shape == (due, len(S.CHANNELS))
        n = self.tuner.next_outputs(due)
        assert n == pkg.tuner_outputs(S.NTAPS, S.DECIM, self.seen["rows"], due)
        tun = self.keep("tun", self.tuner.process(rows, out=b["tun"].t[:K]))
        assert tun.shape == (K, n) and tun.stride(0) > n
        lines = self.scopes["tun"].next_lines(n)
        assert lines == pkg.scope_lines(S.SCOPE["nfft"], S.SCOPE["hop"], S.SCOPE["avg"], self.seen["n"], n)
        blk = self.keep("blk", self.blanker.process(tun, out=b["blk"].t[:K, :n]))
        flt = self.keep("flt", self.rxfilter.process(blk, out=b["flt"].t[:K, :n]))
        for name, z in (("tun", tun), ("blk", blk), ("flt", flt)):
            got = self.keep("scope_" + name, self.scopes[name].process(z, out=b["scope_" + name].t))
            assert got.shape == (2, lines, S.SCOPE["nfft"])
        for name, obj, dtype in (("fsk", self.fsk, pkg.fsk_char_dtype()), ("morse", self.morse, pkg.morse_char_dtype())):
            assert obj.max_chars(n) <= cap[name]
            chars, counts, soft = obj.process(flt, b[name + "_chars"].t[:K], b[name + "_counts"].t[0], b[name + ("_d" if name == "fsk" else "_p")].t[:K, :n])
            b[name + "_chars"].written[:K, :obj.max_chars(n)] = True
            b[name + "_counts"].written[:] = True
            self.keep(name + ("_d" if name == "fsk" else "_p"), soft)
            assert soft.shape == (K, n)
            for j, c in enumerate(records(dtype, chars, counts)):
                assert c.size <= obj.max_chars(n)
                self.parts[name + "_chars"][j].append(c)
        car = self.keep("car", self.carrier.process(flt, out=b["car"].t[:K, :n]))
        dem = self.keep("dem", self.demod.process(car, out=b["dem"].t[:K, :n]))
        blocks = self.squelch.next_blocks(n)
        assert blocks == pkg.squelch_blocks(S.SQUELCH["block"], self.seen["n"], n)
        sql, lv, st = self.squelch.process(flt, dem, out=b["sql"].t[:K, :n], levels=b["sql_levels"].t[:K], states=b["sql_states"].t[:K])
        assert lv.shape == st.shape == (K, blocks)
        self.keep("sql", sql), self.keep("sql_levels", lv), self.keep("sql_states", st)
        adp = self.keep("adp", self.adapt.process(sql, out=b["adp"].t[:K, :n]))
        dns = self.keep("dns", self.denoise.process(adp, out=b["dns"].t[:K, :n]))
        eq = self.keep("eq", self.eq.process(dns, out=b["eq"].t[:K, :n]))
        for v in (blk, flt, car, dem, sql, adp, dns, eq):
            assert v.shape == (K, n) and v.stride(0) > n
        na = self.audio.next_outputs(n)
        assert na == pkg.audio_outputs(S.AUDIO["L"], S.AUDIO["M"], self.seen["n"], n)
        aud, pcm = self.audio.process(eq, out_f32=b["aud"].t[:K], out_i16=b["pcm"].t[:K])
        assert aud.shape == pcm.shape == (K, na) and aud.stride(0) > na
        self.keep("aud", aud), self.keep("pcm", pcm)
        nm = self.mixer.next_outputs(na)
        assert nm == pkg.mixer_outputs(S.MIX_BLOCK, self.seen["na"], na)
        mix, mpcm = self.mixer.process(aud, out_f32=b["mix"].t[:2], out_i16=b["mix_pcm"].t[:cap["nm"]])
        assert mix.shape == (2, nm) and mpcm.shape == (nm, 2)
        self.keep("mix", mix), self.keep("mix_pcm", mpcm, axis=0)
        # behind the last stage of the batch every view still holds what its stage wrote: no later stage wrote over it
        for name, view, host in self.live:
            assert view.cpu().numpy().tobytes() == host.tobytes(), name
        self.seen = dict(ns=self.seen["ns"] + ns, rows=self.seen["rows"] + due, n=self.seen["n"] + n, na=self.seen["na"] + na)
        return types.SimpleNamespace(flt=flt, aud=aud)

    def result(self):
        """every batch's arrays joined, the statuses, and the totals against the closed forms"""
        pkg = self.pkg
        D = {}
        for name, parts in self.parts.items():
            if name in ("fsk_chars", "morse_chars"):
                D[name] = [np.concatenate(p) for p in parts]
            else:
                D[name] = np.concatenate(parts, axis=0 if name in ("rows", "mix_pcm") else 1)
        D["blanker_status"], D["carrier_status"], D["squelch_status"] = self.blanker.read(), self.carrier.read(), self.squelch.read()
        D["mixer_status"], D["fsk_status"], D["morse_status"] = self.mixer.read(), self.fsk.read(), self.morse.read()
        D["adapt_weights"], D["denoise_noise"], D["eq_state"] = self.adapt.read_weights(), self.denoise.read_noise(), self.eq.read_state()
        D["mix_chunk"] = pkg.mixer_chunk()
        assert self.seen["ns"] == S.NS
        assert D["rows"].shape[0] == pkg.channelizer_rows(S.M, S.HOP, S.PROTO.size, 0, S.NS) == S.NROWS
        assert D["tun"].shape[1] == pkg.tuner_outputs(S.NTAPS, S.DECIM, 0, S.NROWS) == S.NRX
        assert D["aud"].shape[1] == pkg.audio_outputs(S.AUDIO["L"], S.AUDIO["M"], 0, S.NRX) == NA
        assert D["mix"].shape[1] == pkg.mixer_outputs(S.MIX_BLOCK, 0, NA) == NM
        assert D["sql_levels"].shape[1] == pkg.squelch_blocks(S.SQUELCH["block"], 0, S.NRX) == NBLOCKS
        assert D["scope_flt"].shape[1] == pkg.scope_lines(S.SCOPE["nfft"], S.SCOPE["hop"], S.SCOPE["avg"], 0, S.NRX) == NLINES
        return D

    def close(self):
        for obj in [self.morse, self.fsk, *self.scopes.values(), self.mixer, self.audio, self.eq, self.denoise, self.adapt, self.squelch,
                    self.demod, self.carrier, self.rxfilter, self.blanker, self.tuner, self.ch]:
            obj.close()


@pytest.fixture(scope="module")
def packed(pkg, dev):
    """the scene, packed on the device as the mixer's end-to-end test packs its own"""
    import torch
    return pkg.pack24_f32(torch.from_numpy(S.scene().copy()).to(dev))


@pytest.fixture(scope="module")
def one(pkg, dev, packed):
    """the scene in one batch: the arrays, the arena's verdict, and the two side runs the radio facts ask for (k's row
    through a receiver without REVERSE, the mixer with NaN in the receivers at gain 0)"""
    import torch
    st = Station(pkg, dev, S.NS)
    last = st.batch(packed)
    D = st.result()
    plain = pkg.Fsk(S.FSK_BANK, S.FSK_PLAIN_SEL, S.FSK_W)
    chars, counts = plain.process(last.flt[S.RX["k"]:S.RX["k"] + 1])
    D["fsk_plain"] = records(pkg.fsk_char_dtype(), chars, counts)[0]
    plain.close()
    poisoned = last.aud.clone()
    poisoned[S.SILENT] = float("nan")
    m = pkg.Mixer(S.GAINS, S.MIX_RAMP, limit=S.MIX_LIMIT)
    D["mix_nan"] = m.process(poisoned).cpu().numpy()
    m.close()
    torch.cuda.synchronize()
    D["damage"] = st.arena.intact()
    st.close()
    return D


@pytest.fixture(scope="module")
def cut(pkg, dev, packed):
    """the same scene through fresh objects, cut at ENDS"""
    import torch
    assert sum(CUTS) == S.NS and all(c % 8 == 0 for c in CUTS) and CUTS[0] == 0 and 0 < CUTS[1] < S.HOP
    st = Station(pkg, dev, max(CUTS))
    off = 0
    for c in CUTS:
        st.batch(packed[6 * off:6 * (off + c)])
        off += c
    D = st.result()
    torch.cuda.synchronize()
    D["damage"] = st.arena.intact()
    st.close()
    return D


@pytest.fixture(scope="module")
def verdict(O, one, packed):
    """section 4.1 on the one-batch run, computed once: (figures, failures, the unpacked stream)"""
    x = O.unpack24_f32(packed.cpu().numpy()).reshape(-1, 2)
    x = x[:, 0].astype(np.float64) + 1j * x[:, 1]
    figures, failures = S.check_stages(one, x)
    return figures, failures


def test_helpers_give_the_station_its_parameters(pkg):
    """the package's design helpers give the arrays station_ref states through the references' restatements"""
    assert np.array_equal(pkg.tuner_prototype(S.M, S.CH["proto_taps"]), S.PROTO)
    assert np.array_equal(pkg.tuner_lowpass(S.NTAPS, S.DECIM), S.LOWPASS)
    assert np.array_equal(pkg.rxfilter_bank(S.RATE, S.WIDTHS, S.FILTER_TAPS), S.BANK)
    assert np.array_equal(pkg.carrier_hilbert(31), S.HILBERT) and pkg.carrier_loop(30.0, S.RATE) == S.CR.loop_gains(30.0, S.RATE)
    assert np.array_equal(pkg.audio_prototype(S.AUDIO["P"], S.AUDIO["T"], 0.45), S.AUDIO_PROTO)
    assert pkg.audio_ratio(S.FS, S.HOP, S.DECIM, 48000) == (S.AUDIO["L"], S.AUDIO["M"])
    assert np.allclose(list(pkg.eq_deemphasis(S.RATE, S.FM_TAU)), S.DEEMPHASIS, rtol=1e-12, atol=1e-15)
    assert np.allclose(list(pkg.eq_section(pkg.PDDC_EQ_LOWPASS, S.RATE, 3000.0)), S.HIGH_CUT, rtol=1e-12, atol=1e-15)
    for got, want in zip(pkg.fsk_modem(S.RATE, S.RATE / 16, S.FR.MARK * S.RATE, S.FR.SPACE * S.RATE, S.FSK_W), S.FSK_BANK[0]):
        assert np.array_equal(got, want)
    for spd, want in zip((16, 40), (S.MORSE_BANK[0], S._KEYERS["m"])):
        for g, w in zip(pkg.morse_keyer(spd * 20.0 / 1.2, 20.0, S.MORSE_W), want):
            assert np.array_equal(g, w)
    assert S.GAINS[0] == list(pkg.mixer_pan(S.GAIN_DB["a"], -1.0)) and pkg.demod_ssb_words(
        S.FS, S.RATE, S._hz(S.CARRIER_WORDS["c"]), *S.SSB_BAND, upper=False) == (S.WORDS[S.RX["cm"]], S.BFO["cm"])


def test_stage_by_stage(verdict):
    """4.1: every stage of the one-batch run against its reference on the device's own arrays of its predecessors; the
    exact stages by their bytes, the float stages within TOL_STATION, no receiver left out of Fsk's and Morse's exact
    comparison"""
    figures, failures = verdict
    for k in sorted(figures):
        print(f"station 4.1: {k:12s} device {figures[k]:.3e}  model {S.MODEL_WORST_STATION[k]:.3e}  TOL_STATION {S.TOL_STATION[k]:.3e}")
    assert failures == [], failures


def test_cut_invariance(one, cut):
    """4.2: every intermediate row, every final product and every status of the cut run has the bytes of the one-batch run"""
    for name, want in one.items():
        if name in ("damage", "mix_chunk", "fsk_plain", "mix_nan"):
            continue
        got = cut[name]
        if isinstance(want, list):
            assert len(got) == len(want) and all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), name
        else:
            assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes(), \
                (name, got.shape, want.shape)


@pytest.mark.parametrize("fact", list(S.FACTS))
def test_radio_fact(one, fact):
    """4.3: the radio facts of tests/test_station_cpu.py on the device's arrays"""
    print(fact, S.FACTS[fact](one))


def test_nothing_outside_the_rows(one, cut):
    """4.4: padding, spare rows and the gaps between the stages' blocks hold never_read after both runs"""
    assert one["damage"] == [] and cut["damage"] == [], (one["damage"], cut["damage"])


def test_controls(one, verdict):
    """4.5: on copies of the downloaded arrays, two receivers' rows swapped between RxFilter and Demod make the Demod
    comparison fail and no other; the squelch's a one sample late against z makes the Squelch comparison fail and no
    other.  Host arithmetic only."""
    assert verdict[1] == []
    for stage, inputs in S.controls(one).items():
        _, failures = S.check_stages(one, only=(stage,), inputs={stage: inputs})
        assert [f[0] for f in failures] == [stage], (stage, failures)
