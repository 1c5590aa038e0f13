"""References for the wideband blanker (include/perseus_ddc.h, pddc_wblank_*), the inputs of its tests and their cut lists.

wblank_fast   vectorised numpy: int64 / uint64 arrays, block sums by reshape, the sliding minimum by H shifted copies, the
              nearest trigger by searchsorted.
wblank_plain  the contract restated sample by sample in Python integers: one loop over the inputs for metering and
              triggers, one over the triggers for the gate.
Both take the whole stream at once with a schedule of settings [(from_sample, thr16, on), ...] (set() between batches)
and give the same dictionary: out (uint8, 6 bytes per input sample), t (the trigger flags), num (the gate numerator per
INPUT sample, -1 open), triggers, blanked, mean (the reference of the block the next sample falls into).
No GPU, no library."""
import numpy as np

NO_BLOCK = (1 << 64) - 1


def unpack_codes(packed):
    """uint8 [6 n] -> (I, Q) int64 codes in [-2^23, 2^23): three bytes each, little-endian, I first"""
    b = np.asarray(packed, dtype=np.uint8).reshape(-1, 6).astype(np.int64)
    i = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    q = b[:, 3] | (b[:, 4] << 8) | (b[:, 5] << 16)
    return i - ((i >> 23) << 24), q - ((q >> 23) << 24)


def pack_codes(i, q):
    """(I, Q) integer codes -> uint8 [6 n]"""
    i = np.asarray(i, dtype=np.int64) & 0xFFFFFF
    q = np.asarray(q, dtype=np.int64) & 0xFFFFFF
    out = np.empty((i.size, 6), dtype=np.uint8)
    for k in range(3):
        out[:, k] = (i >> (8 * k)) & 0xFF
        out[:, 3 + k] = (q >> (8 * k)) & 0xFF
    return out.reshape(-1)


def delay_of(W, r):
    return W + (1 << r) - 1


def _settings(n, sched):
    thr = np.empty(n, dtype=np.uint64)
    on = np.empty(n, dtype=bool)
    sched = sorted(sched)
    assert sched and sched[0][0] == 0
    for j, (m0, t16, o) in enumerate(sched):
        m1 = sched[j + 1][0] if j + 1 < len(sched) else n
        thr[m0:m1] = t16
        on[m0:m1] = bool(o)
    return thr, on


def wblank_fast(packed, B, H, W, r, sched=((0, 256, True),)):
    I, Q = unpack_codes(packed)
    n = I.size
    b = B.bit_length() - 1
    assert B == 1 << b
    D = delay_of(W, r)
    p = (I * I + Q * Q).astype(np.uint64)
    nb = n // B
    S = p[:nb * B].reshape(nb, B).sum(axis=1, dtype=np.uint64)
    pad = np.concatenate([np.full(H, NO_BLOCK, dtype=np.uint64), S])
    least = np.full(nb + 1, NO_BLOCK, dtype=np.uint64)
    for h in range(1, H + 1):                          # block k looks at pad[k + H - h] = S[k - h]
        least = np.minimum(least, pad[H - h:H - h + nb + 1])
    mean = least >> np.uint64(b)
    mean[0] = 0
    thr, on = _settings(n, sched)
    ms = mean[np.arange(n) >> b]
    t = on & (ms > 0) & (p > ((ms * thr) >> np.uint64(4)))
    idx = np.flatnonzero(t)
    num = np.full(n, -1, dtype=np.int64)
    if idx.size:
        c = np.arange(n)
        pos = np.searchsorted(idx, c)
        left = np.where(pos > 0, c - idx[np.maximum(pos - 1, 0)], 1 << 40)
        right = np.where(pos < idx.size, idx[np.minimum(pos, idx.size - 1)] - c, 1 << 40)
        dist = np.minimum(left, right)
        near = dist <= D
        num[near] = np.maximum(dist[near] - W, 0)
    gi, gq = I.copy(), Q.copy()
    g = num >= 0
    for v in (gi, gq):
        v[g] = np.sign(v[g]) * ((np.abs(v[g]) * num[g]) >> r)
    oi, oq = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    oi[D:], oq[D:] = gi[:n - D], gq[:n - D]
    return dict(out=pack_codes(oi, oq), t=t, num=num, triggers=int(t.sum()), blanked=int(g[:max(n - D, 0)].sum()),
                mean=int(mean[n >> b]))


def wblank_plain(packed, B, H, W, r, sched=((0, 256, True),)):
    I, Q = unpack_codes(packed)
    I, Q = [int(v) for v in I], [int(v) for v in Q]
    n = len(I)
    b = B.bit_length() - 1
    D = delay_of(W, r)
    sched = sorted(sched)
    si, thr16, on = -1, 0, False
    s, sums, mean, t = 0, [], 0, [False] * n
    trig = []
    for m in range(n):
        while si + 1 < len(sched) and sched[si + 1][0] <= m:
            si += 1
            thr16, on = int(sched[si][1]), bool(sched[si][2])
        p = I[m] * I[m] + Q[m] * Q[m]
        assert p <= 1 << 47 and mean * thr16 <= 1 << 63
        if on and mean > 0 and p > ((mean * thr16) >> 4):
            t[m] = True
            trig.append(m)
        s += p
        if (m + 1) % B == 0:
            sums.append(s)
            s = 0
            mean = min(sums[-H:]) >> b
    dist = [None] * n
    for u in trig:
        for c in range(max(0, u - D), min(n, u + D + 1)):
            d = abs(c - u)
            if dist[c] is None or d < dist[c]:
                dist[c] = d
    num = [-1] * n
    oi, oq = [0] * n, [0] * n
    blanked = 0
    for k in range(n):                                  # output k is input c = k - D
        c = k - D
        if c < 0:
            continue
        vi, vq = I[c], Q[c]
        if dist[c] is not None:
            blanked += 1
            num[c] = 0 if dist[c] <= W else dist[c] - W
            vi = (1 if vi >= 0 else -1) * ((abs(vi) * num[c]) >> r)
            vq = (1 if vq >= 0 else -1) * ((abs(vq) * num[c]) >> r)
        oi[k], oq[k] = vi, vq
    for c in range(max(n - D, 0), n):                   # gated, not yet given out
        if dist[c] is not None:
            num[c] = 0 if dist[c] <= W else dist[c] - W
    return dict(out=pack_codes(oi, oq), t=np.array(t, dtype=bool), num=np.array(num, dtype=np.int64), triggers=len(trig),
                blanked=blanked, mean=mean)


# ---- inputs ------------------------------------------------------------------------------------------------------------
N_SMALL = 48000
N_LARGE = 1 << 22
PARAM_SETS = [(64, 1, 0, 0), (64, 4, 2, 2), (256, 8, 4, 3), (4096, 16, 128, 7), (4096, 2, 3, 1)]
# a delay longer than a block (D = 255 > B = 64): the outputs in front of the stream's first input (n < D) lie within D of
# triggers from the second block on, and are not blanked outputs -- they are made from no input
PARAM_DEEP = (64, 4, 128, 7)
# the last set of the GPU tests is "one with B > n": it runs on the first N_SHORT samples of the stream
N_SHORT = 4088
THRS = [1.0, 4.0, 16.0, 4096.0]
IMPULSE = 4000000


def noise_stream(n, seed=7, sigma=2000.0, tone=300.0, f=0.1234):
    """Gaussian noise of `sigma` codes with a tone, as (I, Q) int64 codes"""
    rng = np.random.default_rng(seed)
    ph = 2 * np.pi * f * np.arange(n)
    i = np.rint(rng.normal(0, sigma, n) + tone * np.cos(ph)).astype(np.int64)
    q = np.rint(rng.normal(0, sigma, n) + tone * np.sin(ph)).astype(np.int64)
    return i, q


def impulse_positions(n, tile, extra=()):
    """where the small stream's impulses sit: on a coarse grid, on either side of every tile seam (the run seams are
    among them), close pairs whose neighbourhoods overlap, in the stream's first block, in the first 255 samples behind a
    first block of 64, and on the last samples"""
    pos = set(range(1999, n, 1999))
    for seam in range(tile, n, tile):
        pos.update(((seam - 1, seam), (seam - 3, seam + 5), (seam, seam + 1))[(seam // tile) % 3])
    pos.update((10000, 10003, 10020, 10021, 10300, 10400, 10900))
    pos.update((3, 10))
    pos.update((70, 200))                                  # behind a first block of 64, in front of a delay of 255
    pos.update((n - 1, n - 2, n - 130))
    pos.update(extra)
    return np.array(sorted(p for p in pos if 0 <= p < n), dtype=np.int64)


def small_stream(n=N_SMALL, tile=2048, extra=(), seed=7):
    """noise with full-size impulses at impulse_positions(): -> (packed uint8 [6 n], positions)"""
    i, q = noise_stream(n, seed)
    pos = impulse_positions(n, tile, extra)
    sign = np.where(np.arange(pos.size) % 2, -1, 1)
    i[pos] = IMPULSE * sign
    q[pos] = -IMPULSE * sign + 17
    return pack_codes(i, q), pos


def band_streams(n=1 << 20, seed=11):
    """the band scenario: (clean, dirty) packed streams -- noise sigma 2000 with a tone of amplitude 300 at 0.1234 fs;
    dirty has 3-sample impulses of sigma 3e6 every 20011 samples"""
    i, q = noise_stream(n, seed)
    clean = pack_codes(i, q)
    rng = np.random.default_rng(seed + 1)
    i, q = i.copy(), q.copy()
    for s in range(20011, n - 3, 20011):
        i[s:s + 3] = np.clip(np.rint(rng.normal(0, 3.0e6, 3)), -(1 << 23), (1 << 23) - 1).astype(np.int64)
        q[s:s + 3] = np.clip(np.rint(rng.normal(0, 3.0e6, 3)), -(1 << 23), (1 << 23) - 1).astype(np.int64)
    return clean, pack_codes(i, q)


def large_stream(n=N_LARGE, seed=23):
    """noise with 3-sample impulses every 20011 samples and on the seams of three ragged batches (large_cuts)"""
    i, q = noise_stream(n, seed)
    pos = set()
    for s in range(20011, n - 3, 20011):
        pos.update((s, s + 1, s + 2))
    edge = 0
    for c in large_cuts(n)[:-1]:
        edge += c
        pos.update((edge - 1, edge, edge + 9))
    pos.add(n - 1)
    pos = np.array(sorted(pos), dtype=np.int64)
    i[pos] = IMPULSE
    q[pos] = -IMPULSE
    return pack_codes(i, q), pos


def large_cuts(n=N_LARGE):
    a, b = 1398104, 8 * 174763
    return [a, b, n - a - b]


def floor_db(packed, nfft=4096):
    """(median bin, the tone's bin) of a Hann periodogram of the stream, averaged over its segments, in dB"""
    i, q = unpack_codes(packed)
    z = (i + 1j * q).reshape(-1, nfft) * np.hanning(nfft)
    ps = (np.abs(np.fft.fft(z, axis=1)) ** 2).mean(axis=0)
    return 10 * np.log10(np.median(ps)), 10 * np.log10(ps[int(round(0.1234 * nfft))])


def full_scale_stream(n, B, zero_block=5):
    """every code -2^23 (p = 2^47, S = B 2^47), one block of zeros"""
    i = np.full(n, -(1 << 23), dtype=np.int64)
    q = i.copy()
    i[zero_block * B:(zero_block + 1) * B] = 0
    q[zero_block * B:(zero_block + 1) * B] = 0
    return pack_codes(i, q)


def near_full_scale_stream(n, B):
    """every code -2^23 but one zero sample in every block: S = (B - 1) 2^47, so mean = 2^47 - 2^47 / B lies just under the
    power of every other sample.  At thr16 = 16 the limit is the mean and all of them trigger (from the second block on);
    at thr16 = 17 the limit is above 2^47 and none does: the decision hangs on 64-bit products of about 2^51"""
    i = np.full(n, -(1 << 23), dtype=np.int64)
    i[5::B] = 0
    q = i.copy()
    return pack_codes(i, q)


def cut_list(n, D, B, tile):
    """batch sizes, multiples of 8, that add up to n: 3 tile + 40 (so that the cuts behind it lie where there is a
    reference, and triggers), 0, 8, 16, the multiples of 8 around D and 2 D, B - 8, tile - 8, tile, tile + 8, and the rest"""
    f8 = lambda v: v // 8 * 8
    c8 = lambda v: (v + 7) // 8 * 8
    cuts = [3 * tile + 40, 0, 8, 16, f8(D), c8(D), c8(D) + 8, f8(2 * D), c8(2 * D), c8(2 * D) + 8, 0, B - 8, tile - 8, tile,
            tile + 8]
    assert sum(cuts) < n
    return cuts + [n - sum(cuts)]


def cut_edges(cuts):
    return sorted(set(int(e) for e in np.cumsum(cuts)[:-1]))


def cut_stream(params, tile=2048):
    """the small stream with an impulse on the last sample in front of every cut of cut_list() and on the third behind it:
    -> (packed, cuts, edges)"""
    B, H, W, r = params
    cuts = cut_list(N_SMALL, delay_of(W, r), B, tile)
    edges = cut_edges(cuts)
    packed, _ = small_stream(extra=[e - 1 for e in edges] + [e + 2 for e in edges])
    return packed, cuts, edges
