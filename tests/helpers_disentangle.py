"""Float64 numpy restatement of the six disentanglement entry points (include/fadernets.h: fn_column_range, fn_bin_columns, fn_joint_hist,
fn_column_ranks, fn_column_corr, fn_mi_scores) with every fp64 sum in the header's stated order, the mutated variants the device must be told apart
from, the case list, the blobs of the stand-alone twin driver, the comparison of a backend's outputs with the restatement, and stand-in ops for the
Python layer.  Nothing here reads the code under test."""
import numpy as np
import torch

CELLS = 4096
HIST_CHUNK = 4096          # FN_DIS_HIST_CHUNK: the tests straddle it (and read the header's value against this one)
FLT_MAX = np.float32(3.4028234663852886e38)
ULP = 2.0 ** -52
CANARY = np.float32(-777.25)


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------------------
def range_ref(x):
    """x (N, P) float32 -> lo, hi float32 (P,) over the finite entries (a zero as +0.0; +inf / -inf without one), status int32 (P,)"""
    v = x + np.float32(0.0)
    fin = np.isfinite(v)
    lo = np.where(fin, v, np.float32(np.inf)).min(axis=0).astype(np.float32)
    hi = np.where(fin, v, np.float32(-np.inf)).max(axis=0).astype(np.float32)
    return lo, hi, (~fin).any(axis=0).astype(np.int32)


def bin_ref(x, lo, hi, bins, card=None, edge="floor"):
    """-> (img uint8 (P, N), bad int32 (P,): 2 where a discrete column holds a value that is no level).  edge="ceil" is the off-by-one mutation: a
    value exactly on an interior edge falls into the lower bin."""
    N, P = x.shape
    img, bad = np.zeros((P, N), np.uint8), np.zeros(P, np.int32)
    for c in range(P):
        C = 0 if card is None else int(card[c])
        v = x[:, c]
        if C:
            ok = (v >= 0) & (v < np.float32(C)) & (v == np.floor(v))
            img[c] = np.where(ok, v, 0).astype(np.int64)
            bad[c] = 0 if ok.all() else 2
            continue
        if hi[c] == lo[c]:
            continue
        with np.errstate(all="ignore"):
            t = (v.astype(np.float64) - np.float64(lo[c])) / (np.float64(hi[c]) - np.float64(lo[c])) * np.float64(bins)
            whole = np.floor(t) if edge == "floor" else np.maximum(np.ceil(t) - 1.0, 0.0)
            b = np.where(t >= bins, bins - 1, np.where(t >= 0, whole, 0.0))
        img[c] = np.where(np.isnan(t), 0, b).astype(np.int64)
    return img, bad


def hist_ref(bz, bf, drop_row=False, drop_col=False):
    """bz (D, N), bf (A, N) uint8 -> counts int32 (D, A, 64, 64).  drop_row: the last row is not counted; drop_col: the last code column is not"""
    D, A = bz.shape[0], bf.shape[0]
    n = bz.shape[1] - (1 if drop_row else 0)
    out = np.zeros((D, A, CELLS), np.int32)
    for d in range(D - (1 if drop_col else 0)):
        for a in range(A):
            out[d, a] = np.bincount((bz[d, :n] & 63).astype(np.int64) * 64 + (bf[a, :n] & 63), minlength=CELLS)
    return out.reshape(D, A, 64, 64)


def ranks_ref(x, le=False, tie_once=False):
    """x (N, P) float32 without NaN -> mid-ranks float32 (P, N): #less + (#equal + 1) / 2, by counting in the sorted column (a search compares with
    `<` only, so -0.0 ties 0.0).  le: `<=` for `<`; tie_once: a tie group counts as one"""
    N, P = x.shape
    out = np.zeros((P, N), np.float32)
    for c in range(P):
        s = np.sort(x[:, c])
        less, upto = np.searchsorted(s, x[:, c], "left"), np.searchsorted(s, x[:, c], "right")
        equal = upto - less
        if le:
            less = upto
        if tie_once:
            equal = np.ones_like(equal)
        out[c] = ((2 * less + equal + 1).astype(np.float32) * np.float32(0.5))
    return out


def ranks_by_definition(col):
    """the N^2 form on one column, for the known-answer tests"""
    col = np.asarray(col, np.float32)
    less = (col[None, :] < col[:, None]).sum(1)
    equal = (col[None, :] == col[:, None]).sum(1)
    return ((2 * less + equal + 1).astype(np.float32) * np.float32(0.5))


def butterfly(acc):
    """acc (64, ...) -> the value every lane holds after s[l] += s[l ^ o], o = 32 .. 1"""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[idx ^ o]
    return acc[0]


def lane_sum(terms):
    """terms (N, ...) float64 -> lane l adds its rows l, l + 64, ... ascending from 0.0, then the butterfly (an absent row adds +0.0: the same bits)"""
    N = terms.shape[0]
    rows = -(-N // 64)
    pad = np.zeros((rows * 64,) + terms.shape[1:], np.float64)
    pad[:N] = terms
    blk = pad.reshape((rows, 64) + terms.shape[1:])
    acc = np.zeros((64,) + terms.shape[1:], np.float64)
    for k in range(rows):
        acc = acc + blk[k]
    return butterfly(acc)


def corr_ref(X, Y):
    """X (N, P), Y (N, Q) float32 -> dict of mean_x, ss_x (P,), mean_y, ss_y (Q,), cross (P, Q) float64 in the header's order, and under "mag" the
    sums of |term| the bounds are stated in"""
    N = X.shape[0]
    x, y = X.astype(np.float64), Y.astype(np.float64)
    mx, my = lane_sum(x) / np.float64(N), lane_sum(y) / np.float64(N)
    dx, dy = x - mx, y - my
    txy = dx[:, :, None] * dy[:, None, :]
    out = dict(mean_x=mx, ss_x=lane_sum(dx * dx), mean_y=my, ss_y=lane_sum(dy * dy), cross=lane_sum(txy))
    out["mag"] = dict(mean_x=np.abs(x).sum(0) / N, ss_x=(dx * dx).sum(0), mean_y=np.abs(y).sum(0) / N, ss_y=(dy * dy).sum(0), cross=np.abs(txy).sum(0))
    return out


def corr_k(N):
    """the rounding counts of the header: means ceil(N / 64) + 7, centred sums ceil(N / 64) + 9"""
    r = -(-N // 64)
    return dict(mean_x=r + 7, mean_y=r + 7, ss_x=r + 9, ss_y=r + 9, cross=r + 9)


K_I, K_H = 73, 10


def mi_ref(counts):
    """counts (pairs, 64, 64) int -> dict of scores (pairs, 3) float64 (I, H_z, H_f in the header's order), hits int32 (pairs,), mag (pairs, 3)"""
    n = counts.astype(np.int64)
    r, c = n.sum(2), n.sum(1)
    T = r.sum(1)
    hits = np.maximum(n, 0).max(2).sum(1).astype(np.int32)
    pairs = n.shape[0]
    scores, mag = np.zeros((pairs, 3)), np.zeros((pairs, 3))
    for e in range(pairs):
        if T[e] == 0:
            continue
        dT = np.float64(T[e])
        with np.errstate(divide="ignore", invalid="ignore"):
            arg = (n[e] * T[e]).astype(np.float64) / (r[e][:, None] * c[e][None, :]).astype(np.float64)
            term = np.where(n[e] > 0, (n[e].astype(np.float64) / dT) * np.log(np.where(n[e] > 0, arg, 1.0)), 0.0)
            pz, pf = r[e].astype(np.float64) / dT, c[e].astype(np.float64) / dT
            tz = np.where(r[e] > 0, pz * np.log(np.where(r[e] > 0, pz, 1.0)), 0.0)
            tf = np.where(c[e] > 0, pf * np.log(np.where(c[e] > 0, pf, 1.0)), 0.0)
        acc = np.zeros(64)
        for bz in range(64):          # lane bf adds its cells bz ascending
            acc = acc + term[bz]
        scores[e] = butterfly(acc), -butterfly(0.0 + tz), -butterfly(0.0 + tf)
        mag[e] = np.abs(term).sum(), np.abs(tz).sum(), np.abs(tf).sum()
    return dict(scores=scores, hits=hits, mag=mag)


def within(got, want, k, mag, what):
    """|got - want| <= k * 2^-52 * mag, elementwise -> the worst share of the bound in use (0 where the bound is 0 and the values agree)"""
    got, want, mag = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(mag, np.float64)
    err, bound = np.abs(got - want), k * ULP * mag
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float(err.max()), float(bound.flat[int(np.argmax(err - bound))]))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0).max()) if err.size else 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the derived figures, for the planted structure (numpy, from the restatement's or a backend's matrices)
# ------------------------------------------------------------------------------------------------------------------------------
def figures_ref(codes, factors, card, bins):
    """the whole pipeline on the restatement -> dict(mi (D, A), h_factor (A,), r2, rho (D, A), accuracy (D, A))"""
    N, D = codes.shape
    A = factors.shape[1]
    lo, hi, _ = range_ref(codes)
    flo, fhi, _ = range_ref(factors)
    bz, _ = bin_ref(codes, lo, hi, bins)
    bf, _ = bin_ref(factors, flo, fhi, bins, card)
    m = mi_ref(hist_ref(bz, bf).reshape(D * A, 64, 64))
    sc = m["scores"].reshape(D, A, 3)
    raw, rk = corr_ref(codes, factors), corr_ref(ranks_ref(codes).T, ranks_ref(factors).T)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = raw["cross"] / np.sqrt(raw["ss_x"][:, None] * raw["ss_y"][None, :])
        rho = rk["cross"] / np.sqrt(rk["ss_x"][:, None] * rk["ss_y"][None, :])
    return dict(mi=sc[:, :, 0], h_factor=sc[0, :, 2], h_code=sc[:, 0, 1], r2=r * r, rho=rho, accuracy=m["hits"].reshape(D, A) / N)


def planted(seed, N=2048, D=6):
    """the issue's recipe -> codes (N, D), factors (N, 2) float32, card [0, 3]"""
    g = np.random.default_rng(seed)
    f0 = g.random(N)
    f1 = g.integers(0, 3, N)
    z = g.standard_normal((N, D))
    z[:, 3] = f0 + 0.05 * g.standard_normal(N)
    z[:, 1] = np.exp(2 * f0)
    z[:, 5] = f1 + 0.2 * g.standard_normal(N)
    return z.astype(np.float32), np.stack([f0, f1.astype(np.float64)], 1).astype(np.float32), [0, 3]


def check_planted(fig, tag=""):
    """the issue's conditions on the planted structure; fig: mi, r2, rho, accuracy (6, 2) and h_factor (2,) -> the figures it prints"""
    mi0, r20, rho0, acc1 = fig["mi"][:, 0], fig["r2"][:, 0], np.abs(fig["rho"][:, 0]), fig["accuracy"][:, 1]
    rest = [0, 2, 4, 5]
    assert mi0[1] > 2.2 and mi0[3] > 1.4 and (mi0[rest] < 0.15).all(), (tag, mi0)
    assert int(np.argmax(mi0)) == 1 and int(np.argmax(rho0)) == 1 and int(np.argmax(r20)) == 3, (tag, mi0, rho0, r20)
    assert r20[3] > 0.96 and (r20[rest] < 0.01).all(), (tag, r20)
    assert rho0[3] > 0.98 and (rho0[rest] < 0.1).all(), (tag, rho0)
    mi1 = np.sort(fig["mi"][:, 1])
    mig1 = (mi1[-1] - mi1[-2]) / fig["h_factor"][1]
    assert mig1 > 0.9 and int(np.argmax(fig["mi"][:, 1])) == 5, (tag, mig1)
    assert acc1[5] > 0.98 and (acc1[:5] < 0.42).all(), (tag, acc1)
    return dict(mi_1=mi0[1], mi_3=mi0[3], mi_rest=mi0[rest].max(), mig_f1=mig1, acc_rest=acc1[:5].max())


# ------------------------------------------------------------------------------------------------------------------------------
# the case list
# ------------------------------------------------------------------------------------------------------------------------------
def _column(g, kind, N, bins):
    if kind == 0:
        return g.standard_normal(N)
    if kind == 1:          # ties, with both zeros
        v = np.round(g.standard_normal(N) * 2) / 2
        v[v == 0] = np.where(g.random(int((v == 0).sum())) < 0.5, -0.0, 0.0)
        return v
    if kind == 2:          # exactly on the bin edges: lo = 0, hi = bins (both present from N = 2), t = x
        v = g.integers(0, bins + 1, N).astype(np.float64)
        v[0], v[-1] = 0.0, bins
        return v
    if kind == 3:          # the ends of the format
        return g.choice(np.array([FLT_MAX, -FLT_MAX, 1e-45, -1e-45, 0.0, -0.0, 1.0, -2.5, 1.1754942e-38]), N)
    return np.full(N, 0.75)          # constant


def make_case(N, D, A, bins, card, seed, pad_z=0, pad_f=0, off_z=0, off_f=0):
    """codes live at columns [off_z, off_z + D) of a float32 buffer (N, off_z + D + pad_z) filled with canaries, factors likewise; factor a is discrete
    with card[a] levels where card[a] > 0.  Column c of the codes is of kind (c + seed) % 5."""
    g = np.random.default_rng(1000 + seed)
    zbuf = np.full((N, off_z + D + pad_z), CANARY, np.float32)
    fbuf = np.full((N, off_f + A + pad_f), CANARY, np.float32)
    for c in range(D):
        zbuf[:, off_z + c] = _column(g, (c + seed) % 5, N, bins).astype(np.float32)
    for a in range(A):
        if card[a]:
            v = g.integers(0, card[a], N).astype(np.float32)
            v[-1] = card[a] - 1
        else:
            v = _column(g, (0, 2, 1)[(a + seed) % 3], N, bins).astype(np.float32)
        fbuf[:, off_f + a] = v
    return dict(tag="N%d D%d A%d bins%d card%s seed%d" % (N, D, A, bins, card, seed), N=N, D=D, A=A, bins=bins, card=list(card), zbuf=zbuf, fbuf=fbuf,
                off_z=off_z, off_f=off_f, n_pad=-(-N // 64) * 64 if seed % 2 else N + seed % 5)


def cases():
    """every N, D, A, bins and card of the list at least once; row strides above the width and column slices in most"""
    Ns = [1, 2, 63, 64, 65, 255, 256, 257, 513, HIST_CHUNK - 1, HIST_CHUNK, HIST_CHUNK + 1]
    Ds, binss, cards = [1, 2, 5, 65], [1, 2, 20, 64], [1, 2, 64]
    out = []
    for k, N in enumerate(Ns):
        D = Ds[k % 4] if N < 1000 else (2, 5, 1)[k % 3]
        A = (1, 3)[k % 2]
        card = [0, cards[k % 3], 0][:A] if A == 3 else [(0, cards[k % 3])[k % 4 == 1]]
        out.append(make_case(N, D, A, binss[(k + k // 4) % 4], card, k, pad_z=(0, 3)[k % 3 > 0], pad_f=k % 2, off_z=(0, 2)[k % 3 == 2], off_f=(0, 1)[k % 4 == 3]))
    out.append(make_case(257, 65, 3, 64, [64, 0, 1], 12, pad_z=1, off_z=1))
    out.append(make_case(64, 5, 3, 20, [0, 0, 2], 13, pad_f=2, off_f=1))
    return out


def views(c):
    z = c["zbuf"][:, c["off_z"]:c["off_z"] + c["D"]]
    f = c["fbuf"][:, c["off_f"]:c["off_f"] + c["A"]]
    return z, f


# ------------------------------------------------------------------------------------------------------------------------------
# a backend's pipeline against the restatement.  A backend offers, on numpy arrays:
#   range(buf, off, P) -> lo, hi, status           bins(buf, off, P, lo, hi, bins, card, n_pad, status) -> img (P, n_pad), status
#   hist(bz, bf, N) -> counts (D, A, 64, 64)       ranks(buf, off, P, n_pad) -> (P, n_pad) float32
#   corr(xflat, x_rs, x_cs, P, yflat, y_rs, y_cs, Q, N) -> mean_x, ss_x, mean_y, ss_y, cross (P, Q)
#   mi(counts (pairs, 64, 64)) -> scores (pairs, 3), hits
# ------------------------------------------------------------------------------------------------------------------------------
def run_pipeline(c, be):
    N, D, A, n_pad = c["N"], c["D"], c["A"], c["n_pad"]
    o = {}
    o["lo_z"], o["hi_z"], o["st_z"] = be.range(c["zbuf"], c["off_z"], D)
    o["lo_f"], o["hi_f"], o["st_f"] = be.range(c["fbuf"], c["off_f"], A)
    o["img_z"], o["st_z2"] = be.bins(c["zbuf"], c["off_z"], D, o["lo_z"], o["hi_z"], c["bins"], None, n_pad, o["st_z"])
    o["img_f"], o["st_f2"] = be.bins(c["fbuf"], c["off_f"], A, o["lo_f"], o["hi_f"], c["bins"], c["card"] if any(c["card"]) else None, n_pad, o["st_f"])
    o["counts"] = be.hist(o["img_z"], o["img_f"], N)
    o["scores"], o["hits"] = be.mi(o["counts"].reshape(D * A, 64, 64))
    o["rk_z"], o["rk_f"] = be.ranks(c["zbuf"], c["off_z"], D, n_pad), be.ranks(c["fbuf"], c["off_f"], A, n_pad)
    ldz, ldf = c["zbuf"].shape[1], c["fbuf"].shape[1]
    o["raw"] = be.corr(c["zbuf"].reshape(-1)[c["off_z"]:], ldz, 1, D, c["fbuf"].reshape(-1)[c["off_f"]:], ldf, 1, A, N)
    o["rk"] = be.corr(o["rk_z"].reshape(-1), 1, n_pad, D, o["rk_f"].reshape(-1), 1, n_pad, A, N)
    return o


def reference(c):
    """the restatement of a case, computed once"""
    if "ref" in c:
        return c["ref"]
    z, f = views(c)
    N, D, A = c["N"], c["D"], c["A"]
    r = {}
    r["lo_z"], r["hi_z"], r["st_z"] = range_ref(z)
    r["lo_f"], r["hi_f"], r["st_f"] = range_ref(f)
    r["img_z"], _ = bin_ref(z, r["lo_z"], r["hi_z"], c["bins"])
    r["img_f"], bad = bin_ref(f, r["lo_f"], r["hi_f"], c["bins"], c["card"])
    r["st_f2"] = r["st_f"] | bad
    r["counts"] = hist_ref(r["img_z"], r["img_f"])
    r["mi"] = mi_ref(r["counts"].reshape(D * A, 64, 64))
    r["rk_z"], r["rk_f"] = ranks_ref(z), ranks_ref(f)
    r["raw"], r["rk"] = corr_ref(z, f), corr_ref(r["rk_z"].T, r["rk_f"].T)
    c["ref"] = r
    return r


def check_pipeline(c, o):
    """bit-equal ranges, bin images (the padding untouched), counts, hits and ranks; the fp64 outputs within the header's bounds -> the worst shares"""
    r, N, tag = reference(c), c["N"], c["tag"]
    for k in ("lo_z", "hi_z", "lo_f", "hi_f"):
        assert o[k].dtype == np.float32 and o[k].tobytes() == r[k].tobytes(), (tag, k, o[k], r[k])
    assert np.array_equal(o["st_z"], r["st_z"]) and np.array_equal(o["st_z2"], r["st_z"]) and np.array_equal(o["st_f2"], r["st_f2"]), (tag, "status")
    for k in ("img_z", "img_f"):
        assert np.array_equal(o[k][:, :N], r[k]), (tag, k)
        assert (o[k][:, N:] == 0xEE).all(), (tag, k, "padding written")
    assert o["counts"].dtype == np.int32 and np.array_equal(o["counts"], r["counts"]) and int(o["counts"].sum()) == N * c["D"] * c["A"], (tag, "counts")
    assert np.array_equal(o["hits"], r["mi"]["hits"]), (tag, "hits")
    for k in ("rk_z", "rk_f"):
        assert o[k].dtype == np.float32 and o[k][:, :N].tobytes() == r[k].tobytes(), (tag, k)
        assert (o[k][:, N:] == CANARY).all(), (tag, k, "padding written")
    share = {}
    for j, (name, k) in enumerate((("I", K_I), ("H_z", K_H), ("H_f", K_H))):
        share[name] = within(o["scores"][:, j], r["mi"]["scores"][:, j], k, r["mi"]["mag"][:, j], (tag, name))
    for which in ("raw", "rk"):
        ks = corr_k(N)
        for name, got in zip(("mean_x", "ss_x", "mean_y", "ss_y", "cross"), o[which]):
            share[which + "." + name] = within(got, r[which][name], ks[name], r[which]["mag"][name], (tag, which, name))
    return share


def mutants(c):
    """the restatement's outputs under each mutation -> dict name -> (key of the pipeline's outputs, the mutated array cut to what is compared)"""
    z, f = views(c)
    r = reference(c)
    m = {}
    m["bin edge off by one"] = ("img_z", bin_ref(z, r["lo_z"], r["hi_z"], c["bins"], edge="ceil")[0])
    m["last row dropped"] = ("counts", hist_ref(r["img_z"], r["img_f"], drop_row=True))
    m["last column dropped"] = ("counts", hist_ref(r["img_z"], r["img_f"], drop_col=True))
    m["<= for < in the rank"] = ("rk_z", ranks_ref(z, le=True))
    m["a tie counted once"] = ("rk_z", ranks_ref(z, tie_once=True))
    return m


# ------------------------------------------------------------------------------------------------------------------------------
# the stand-alone twin driver (csrc/host/disentangle_check.cpp) as a backend
# ------------------------------------------------------------------------------------------------------------------------------
def _i32(*v):
    return np.array(list(v) + [0] * (10 - len(v)), np.int32).tobytes()


def _flat(buf, off, N, ld, P):
    return np.ascontiguousarray(buf.reshape(-1)[off:off + (N - 1) * ld + P])


class TwinBackend:
    """run: blob -> the bytes of out.bin"""

    def __init__(self, run):
        self.run = run

    def _out(self, blob):
        raw = self.run(blob)
        rc = int(np.frombuffer(raw[:4], np.int32)[0])
        assert rc == 0, rc
        return raw[4:]

    @staticmethod
    def _image(raw, dtype, P, n_pad, N, fill):
        img = np.full(P * n_pad, fill, dtype)
        flat = np.frombuffer(raw, dtype)
        assert flat.size == (P - 1) * n_pad + N
        img[:flat.size] = flat
        return img.reshape(P, n_pad)

    def range(self, buf, off, P):
        N, ld = buf.shape
        raw = self._out(_i32(0, N, P, ld) + _flat(buf, off, N, ld, P).tobytes())
        f = np.frombuffer(raw[:8 * P], np.float32)
        return f[:P].copy(), f[P:].copy(), np.frombuffer(raw[8 * P:], np.int32).copy()

    def bins(self, buf, off, P, lo, hi, bins, card, n_pad, status):
        N, ld = buf.shape
        blob = _i32(1, N, P, ld, bins, n_pad, 0 if card is None else 1) + _flat(buf, off, N, ld, P).tobytes() + lo.tobytes() + hi.tobytes()
        raw = self._out(blob + (b"" if card is None else np.array(card, np.int32).tobytes()))
        n = (P - 1) * n_pad + N
        return self._image(raw[:n], np.uint8, P, n_pad, N, 0xEE), np.frombuffer(raw[n:], np.int32) | status          # the driver starts status at 0

    def hist(self, bz, bf, N):
        D, A = bz.shape[0], bf.shape[0]
        cut = lambda m: np.ascontiguousarray(m.reshape(-1)[:(m.shape[0] - 1) * m.shape[1] + N])
        raw = self._out(_i32(2, N, D, A, bz.shape[1], bf.shape[1]) + cut(bz).tobytes() + cut(bf).tobytes())
        return np.frombuffer(raw, np.int32).reshape(D, A, 64, 64).copy()

    def ranks(self, buf, off, P, n_pad):
        N, ld = buf.shape
        raw = self._out(_i32(3, N, P, ld, n_pad) + _flat(buf, off, N, ld, P).tobytes())
        return self._image(raw, np.float32, P, n_pad, N, CANARY)

    def corr(self, xf, x_rs, x_cs, P, yf, y_rs, y_cs, Q, N):
        cut = lambda v, rs, cs, C: np.ascontiguousarray(v[:(N - 1) * rs + (C - 1) * cs + 1])
        raw = self._out(_i32(4, N, P, Q, x_rs, x_cs, y_rs, y_cs) + cut(xf, x_rs, x_cs, P).tobytes() + cut(yf, y_rs, y_cs, Q).tobytes())
        v = np.frombuffer(raw, np.float64)
        return v[:P], v[P:2 * P], v[2 * P:2 * P + Q], v[2 * P + Q:2 * P + 2 * Q], v[2 * P + 2 * Q:].reshape(P, Q)

    def mi(self, counts):
        pairs = counts.shape[0]
        raw = self._out(_i32(5, pairs) + np.ascontiguousarray(counts, np.int32).tobytes())
        return np.frombuffer(raw[:24 * pairs], np.float64).reshape(pairs, 3), np.frombuffer(raw[24 * pairs:], np.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# stand-in ops for the Python layer: the six entry points as their restatement on CPU tensors
# ------------------------------------------------------------------------------------------------------------------------------
def dis_fake_ops():
    import helpers_likelihood as hk
    base = type(hk.lik_fake_ops())

    class DisFakeOps(base):
        def column_range(self, x, lo, hi, status):
            self.calls.append("column_range")
            a, b, s = range_ref(x.numpy())
            lo.copy_(torch.from_numpy(a)), hi.copy_(torch.from_numpy(b)), status.copy_(torch.from_numpy(s))

        def bin_columns(self, x, lo, hi, bins, img, status, card=None):
            self.calls.append("bin_columns")
            im, bad = bin_ref(x.numpy(), lo.numpy(), hi.numpy(), bins, card)
            img[:, :x.shape[0]].copy_(torch.from_numpy(im)), status.copy_(status | torch.from_numpy(bad))

        def joint_hist(self, bz, bf, N, counts):
            self.calls.append("joint_hist")
            counts.copy_(torch.from_numpy(hist_ref(bz.numpy()[:, :N], bf.numpy()[:, :N])).view(counts.shape))

        def column_ranks(self, x, ranks):
            self.calls.append("column_ranks")
            xn = x.numpy()
            ranks[:, :x.shape[0]].copy_(torch.from_numpy(np.stack([ranks_by_definition(np.nan_to_num(xn[:, c])) for c in range(xn.shape[1])])))

        def column_corr(self, X, Y, mean_x, ss_x, mean_y, ss_y, cross):
            self.calls.append("column_corr")
            with np.errstate(invalid="ignore"):          # a NaN column is the caller's to report, from the status words
                r = corr_ref(X.numpy(), Y.numpy())
            for t, k in ((mean_x, "mean_x"), (ss_x, "ss_x"), (mean_y, "mean_y"), (ss_y, "ss_y"), (cross, "cross")):
                t.copy_(torch.from_numpy(np.ascontiguousarray(r[k])).view(t.shape))

        def mi_scores(self, counts, out, hits):
            self.calls.append("mi_scores")
            m = mi_ref(counts.numpy().reshape(-1, 64, 64))
            out.copy_(torch.from_numpy(m["scores"]).view(out.shape)), hits.copy_(torch.from_numpy(m["hits"]))

    return DisFakeOps()
