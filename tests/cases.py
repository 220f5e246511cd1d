"""Seeded input builders shared by the CPU (oracle-vs-reference / golden) and GPU (HIP-vs-oracle) tests."""
import numpy as np

from vvcsoftware_vtm_amd.abi import IMV_PU, IMV_RESULT, SAO_DTYPE, SEARCH_BEST as BEST, TZ_CFG, TZ_PU  # noqa: F401


def rand_plane(rng, h, w, bd, kind="uniform"):
    mx = (1 << bd) - 1
    if kind == "uniform":
        return rng.integers(0, mx + 1, (h, w)).astype(np.int16)
    if kind == "flat":      # many equal neighbours (sign == 0 paths)
        return ((rng.integers(0, mx + 1, (h, w)) >> (bd - 3)) + (mx // 2)).astype(np.int16)
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        v = (np.sin(xx / 17.0) + np.cos(yy / 11.0) + 2) / 4 * mx + rng.normal(0, 3 * 2 ** (bd - 8), (h, w))
        return np.clip(np.rint(v), 0, mx).astype(np.int16)
    if kind == "extreme":   # saturating values at both ends (clip paths)
        return rng.choice(np.array([0, 1, mx - 1, mx], dtype=np.int16), (h, w))
    raise ValueError(kind)


def alf_coeffs(rng, amp=60):
    lc = rng.integers(-amp, amp + 1, (25, 13)).astype(np.int16)
    lc[:, 12] = 512 - 2 * lc[:, :12].sum(1)
    cc = rng.integers(-amp, amp + 1, 7).astype(np.int16)
    cc[6] = 512 - 2 * cc[:6].sum()
    return lc, cc


def n_ctus(w, h, cw, ch=None):
    ch = ch or cw
    return ((w + cw - 1) // cw), ((h + ch - 1) // ch)


def sao_params(rng, w, h, cw, ch, full_avail=True, types=None):
    nx, ny = n_ctus(w, h, cw, ch)
    prm = np.zeros(nx * ny, SAO_DTYPE)
    prm["type"] = rng.integers(-1, 5, nx * ny) if types is None else rng.choice(types, nx * ny)
    prm["offset"] = rng.integers(-31, 32, (nx * ny, 32))
    for j in range(ny):
        for i in range(nx):
            L, R, A, B = i > 0, i < nx - 1, j > 0, j < ny - 1
            bits = [L, R, A, B, A and L, A and R, B and L, B and R]
            a = 0
            for k, b in enumerate(bits):
                if b and (full_avail or rng.random() < 0.7):
                    a |= 1 << k
            prm["avail"][j * nx + i] = a
    return prm


# offsets at the edges of the strip form's packed ranges (6-bit EO table, 16-bit sample pairs) and at the int16 extremes
SAO_EDGE_OFFSETS = np.array([-32768, -32767, -33, -32, -31, 30, 31, 32, 32766, 32767], np.int16)


def sao_picture_params(rng, w, h, ctu, mode, full_avail=False):
    """vvcgpu_sao_ctu arrays of the three planes of a 4:2:0 picture (luma w x h, luma CTU ctu).  mode:
      'type<t>'  every CTU of type t (-1..4), offsets drawn per CTU in -31..31 (all 32 entries: BO with every band random)
      'band4'    BO as a decoder binding builds it: four consecutive bands (modulo 32) from a random start, zeros elsewhere
      'mixed'    random types, a quarter of the CTUs with offsets outside the packed EO range
      'edge_eo' / 'edge_bo'   EO / BO types with every offset drawn from SAO_EDGE_OFFSETS"""
    out = []
    for c in range(3):
        pw, ph, cs = (w, h, ctu) if c == 0 else (w // 2, h // 2, ctu // 2)
        if mode.startswith("type"):
            prm = sao_params(rng, pw, ph, cs, cs, full_avail, types=[int(mode[4:])])
        elif mode == "band4":
            prm = sao_params(rng, pw, ph, cs, cs, full_avail, types=[4])
            prm["offset"] = 0
            for r in prm:
                r["offset"][(int(rng.integers(0, 32)) + np.arange(4)) % 32] = rng.integers(-31, 32, 4)
        elif mode == "mixed":
            prm = sao_params(rng, pw, ph, cs, cs, full_avail, types=[-1, 0, 1, 2, 3, 4])
            big = rng.random(prm.size) < 0.25
            prm["offset"][big] = rng.integers(-300, 301, (int(big.sum()), 32))
        elif mode in ("edge_eo", "edge_bo"):
            prm = sao_params(rng, pw, ph, cs, cs, full_avail, types=[0, 1, 2, 3] if mode == "edge_eo" else [4])
            prm["offset"] = rng.choice(SAO_EDGE_OFFSETS, prm["offset"].shape)
        else:
            raise ValueError(mode)
        out.append(prm)
    return out


def ctu_enables(rng, w, h, ctu, p=0.6):
    """one random ALF enable byte per CTU (raster order)"""
    nx, ny = n_ctus(w, h, ctu)
    return (rng.random(nx * ny) < p).astype(np.uint8)


def deblock_maps(rng, w, h, mode="cu"):
    """Edge/BS/QP maps per 4x4 luma unit (see include/vvcgpu.h).  mode 'cu': a seeded quadtree CU grid with
    intra/inter blocks and cbf-like BS; mode 'random': arbitrary map bytes (stress: off-grid edges, flags)."""
    w4, h4 = w // 4, h // 4
    ev = np.zeros((h4, w4), np.uint8)
    eh = np.zeros((h4, w4), np.uint8)
    qpl = np.zeros((h4, w4), np.int8)
    qpc = np.zeros((h4, w4), np.int8)
    if mode == "random":
        ev[:] = rng.integers(0, 64, (h4, w4))
        eh[:] = rng.integers(0, 64, (h4, w4))
        # BS value 3 never occurs in the reference
        for m in (ev, eh):
            m[(m & 3) == 3] &= 0xFE
            m[((m >> 2) & 3) == 3] &= 0xFB
        qpl[:] = rng.integers(0, 64, (h4, w4))
        qpc[:] = rng.integers(0, 64, (h4, w4))
        return ev, eh, qpl, qpc
    intra = np.zeros((h4, w4), bool)

    def split(x, y, s):
        if s > 8 and (s > 64 or rng.random() < 0.55):
            for dy in (0, s // 2):
                for dx in (0, s // 2):
                    split(x + dx, y + dy, s // 2)
            return
        x1, y1 = min(x + s, w), min(y + s, h)
        if x >= w or y >= h:
            return
        ux0, uy0, ux1, uy1 = x // 4, y // 4, x1 // 4, y1 // 4
        isint = rng.random() < 0.3
        intra[uy0:uy1, ux0:ux1] = isint
        q = int(rng.integers(22, 46))
        qpl[uy0:uy1, ux0:ux1] = q
        qpc[uy0:uy1, ux0:ux1] = q if rng.random() < 0.7 else int(rng.integers(22, 46))
        nf = rng.random() < 0.03
        for uy in range(uy0, uy1):          # left border
            if x > 0:
                pi = intra[uy, ux0 - 1] or isint
                bs = 2 if pi else int(rng.integers(0, 2))
                ev[uy, ux0] = bs | ((2 if pi else 0) << 2) | (0x20 if nf else 0)
        for ux in range(ux0, ux1):          # top border
            if y > 0:
                pi = intra[uy0 - 1, ux] or isint
                bs = 2 if pi else int(rng.integers(0, 2))
                eh[uy0, ux] = bs | ((2 if pi else 0) << 2) | (0x10 if nf and rng.random() < 0.5 else 0)

    for y in range(0, h, 128):
        for x in range(0, w, 128):
            split(x, y, 128)
    return ev, eh, qpl, qpc


# ---- N2: integer TZ search ------------------------------------------------------------------------------------------
def tz_planes(rng, W, H, M, bd, motion=(7, -5), noise=3):
    """ref: (H+2M) x (W+2M) blob texture (the padded reference picture); org: the picture displaced by `motion` + noise,
    so that searches have a real optimum away from most start vectors."""
    from scipy.ndimage import gaussian_filter
    mx = (1 << bd) - 1
    f = gaussian_filter(rng.normal(0, 1, (H + 2 * M, W + 2 * M)), 2.5) * 6 + gaussian_filter(rng.normal(0, 1, (H + 2 * M, W + 2 * M)), 9) * 30
    ref = np.clip(np.rint((f * 0.12 + 0.5) * mx), 0, mx).astype(np.int16)
    dx, dy = motion
    org = ref[M + dy:M + dy + H, M + dx:M + dx + W].astype(np.int32) + rng.integers(-noise, noise + 1, (H, W)) * (1 << (bd - 8))
    return np.ascontiguousarray(np.clip(org, 0, mx).astype(np.int16)), ref


def tz_pus(rng, n, W, H, M, sizes, flags_choices=(0, 1, 2, 3, 4, 5), spread=40, sub_mode2=None):
    pus = np.zeros(n, TZ_PU)
    for i in range(n):
        w, h = sizes[int(rng.integers(0, len(sizes)))]
        x = int(rng.integers(0, (W - w) // 4 + 1)) * 4
        y = int(rng.integers(0, (H - h) // 4 + 1)) * 4
        r = pus[i]
        r["org_x"], r["org_y"], r["ref_x"], r["ref_y"], r["pos_x"], r["pos_y"] = x, y, M + x, M + y, x, y
        far = rng.random() < 0.3
        s = spread * 4 if far else 24
        r["start_x"], r["start_y"] = int(rng.integers(-s, s + 1)), int(rng.integers(-s, s + 1))
        r["pred2_x"], r["pred2_y"] = int(rng.integers(-12, 13)), int(rng.integers(-12, 13))
        r["pred_hor"], r["pred_ver"] = int(r["start_x"]) + int(rng.integers(-8, 9)), int(r["start_y"]) + int(rng.integers(-8, 9))
        r["w"], r["h"] = w, h
        m2 = bool(rng.integers(0, 2)) if sub_mode2 is None else sub_mode2
        r["sub_shift"] = 1 if (m2 and h > 8 and w <= 64) else 0
        r["flags"] = flags_choices[int(rng.integers(0, len(flags_choices)))]
    return pus


def tz_cfg(W, H, M, lam, search_range=64, first_stop=0, max_cu=128, cost_scale=2, imv_shift=0, wg_per_pu=0):
    c = np.zeros(1, TZ_CFG)
    c[0] = (lam, cost_scale, imv_shift, search_range, first_stop, W, H, max_cu, max_cu, 0, 0, W + 2 * M, H + 2 * M, wg_per_pu, 0)
    return c


# ---- N2: AMVR integer refinement -----------------------------------------------------------------------------------
def imv_pus(rng, n, W, H, M, sizes, imv_shift):
    """PUs whose AMVP candidates satisfy what the encoder guarantees on entry (mv - cand is a multiple of 4 quarter units)."""
    pus = np.zeros(n, IMV_PU)
    for i in range(n):
        w, h = sizes[int(rng.integers(0, len(sizes)))]
        x = int(rng.integers(0, (W - w) // 4 + 1)) * 4
        y = int(rng.integers(0, (H - h) // 4 + 1)) * 4
        r = pus[i]
        r["org_x"], r["org_y"], r["ref_x"], r["ref_y"], r["pos_x"], r["pos_y"] = x, y, M + x, M + y, x, y
        r["mv_x"], r["mv_y"] = int(rng.integers(-40, 41)), int(rng.integers(-40, 41))
        step = 1 << imv_shift
        for c in range(2):
            r["cand_x"][c] = (int(rng.integers(-60, 61)) * step) // 1 if rng.random() < 0.5 else int(rng.integers(-50, 51)) * 4
            r["cand_y"][c] = int(rng.integers(-50, 51)) * 4
            r["cand_x"][c] = (int(r["cand_x"][c]) // 4) * 4
        if rng.random() < 0.25:
            r["cand_x"][1], r["cand_y"][1] = r["cand_x"][0], r["cand_y"][0]          # equal candidates: the SATD is reused (:2449-2461)
        r["num_cand"] = 2 if rng.random() < 0.85 else 1
        r["mvp_idx"] = int(rng.integers(0, int(r["num_cand"])))
        r["idx_cost"] = (1, 1) if r["num_cand"] == 2 else (0, 0)
        r["bits"] = int(rng.integers(8, 40))
        r["w"], r["h"] = w, h
    return pus


def unpack_plane(lo, hi):
    """inverse of tests/golden/gen_deblock.py:pack_plane: low / high bytes of the horizontal-then-vertical differences modulo 2^16 -> int16 plane"""
    d = lo.astype(np.int64) | (hi.astype(np.int64) << 8)
    v = np.cumsum(np.cumsum(d, axis=0), axis=1) & 0xFFFF
    return v.astype(np.uint16).view(np.int16)


def deblock_golden():
    """-> list of pictures of tests/golden/deblock.npz (the compiled reference's own loopFilterPic: planes in front, the maps its xDeblockCU walk
    produced, slice / PPS parameters, planes behind): dicts with hdr (field -> int), ev, eh, qp_luma, qp_chroma, pre[3], post[3]"""
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "deblock.npz"))
    fields = [str(f) for f in z["hdr_fields"]]
    pics = []
    for i in range(int(z["n"])):
        r = {"hdr": dict(zip(fields, (int(v) for v in z["hdr%d" % i])))}
        for k in ("ev", "eh", "qp_luma", "qp_chroma"):
            r[k] = np.ascontiguousarray(z["%s_%d" % (k, i)])
        r["pre"] = [np.ascontiguousarray(unpack_plane(z["pre%d_lo_%d" % (c, i)], z["pre%d_hi_%d" % (c, i)])) for c in range(3)]
        r["post"] = [(r["pre"][c].astype(np.int32) + z["delta%d_%d" % (c, i)]).astype(np.int16) for c in range(3)]
        pics.append(r)
    return pics


# ---- inputs at the exactness bounds of the transform, quantiser and statistics kernels ------------------------------------
TR_NAMES = ("DCT2", "DCT8", "DST7")
_tr_tables = None


def tr_matrix(t, n):
    """the n-point matrix of transform type t (0 DCT-II, 1 DCT-VIII, 2 DST-VII) of tests/golden/tr_tables.npz, row = frequency"""
    global _tr_tables
    if _tr_tables is None:
        import os
        _tr_tables = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "tr_tables.npz")))
    return _tr_tables["%s_%d" % (TR_NAMES[t], n)].astype(np.int64)


def _sgn(v):
    return np.where(v < 0, -1, 1).astype(np.int64)         # sign(0) counts as +1


def tr_aligned_block(w, h, th, tv, k, l, amp, negate=False):
    """h x w residual whose signs follow row k of the horizontal and row l of the vertical matrix: coefficient (l, k) of the forward transform
    is the largest a block of |x| <= amp can give, and the first stage's sums for frequency k are amp * (row-sum of |c|) in every row"""
    b = amp * np.outer(_sgn(tr_matrix(tv, h)[l]), _sgn(tr_matrix(th, w)[k]))
    return (-b if negate else b).astype(np.int16)


_tr_idx = {}


def _tr_aligned_idx(t, n):
    if (t, n) not in _tr_idx:
        kept = min(n, 32)
        out = []
        for i in (0, int(np.abs(tr_matrix(t, n))[:kept].sum(1).argmax()), kept - 1):
            if i not in out:
                out.append(i)
        _tr_idx[(t, n)] = out
    return _tr_idx[(t, n)]


def tr_aligned_set(w, h, th, tv):
    """(k, l, negate): per dimension index 0, the kept index with the largest row-sum of |c| and the last kept index min(N, 32) - 1, crossed,
    each with and without negation (equal indices once)"""
    for k in _tr_aligned_idx(th, w):
        for l in _tr_aligned_idx(tv, h):
            for negate in (False, True):
                yield k, l, negate


def tr_aligned_coeffs(w, h, th, tv, x, y, val):
    """h x w int32 coefficients: (l, k) = val * sign(Th[k][x]) * sign(Tv[l][y]) inside the kept region (k, l < 32), zero outside: every term of
    output sample (x, y) of the inverse transform has the sign of val"""
    wj, hj = min(w, 32), min(h, 32)
    c = np.zeros((h, w), np.int32)
    c[:hj, :wj] = val * np.outer(_sgn(tr_matrix(tv, h)[:hj, y]), _sgn(tr_matrix(th, w)[:wj, x]))
    return c


def tr_sample_points(w, h):
    """the four corners and one interior sample"""
    return [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2 - (1 if h > 2 else 0))]


TR_WORST_PAIRS = [(0, 0), (1, 1), (1, 2), (2, 1), (2, 2)]
TR_SIZES = (2, 4, 8, 16, 32, 64)


def tr_pair_allowed(w, h, th, tv):
    return (th, tv) == (0, 0) or (4 <= w <= 32 and 4 <= h <= 32)


def tr_worst_rows():
    """forward items (w, h, th, tv, k, l, negate, amp, bd): every W x H in 2..64 with DCT-II / DCT-II and every shape in 4..32 with the other four
    pairs, the patterns of tr_aligned_set, amplitude 1023 at bit depth 10, 255 and 1023 at bit depth 8 (the items of
    tests/golden/transform_worst.npz)"""
    rows = []
    for bd, amps in ((10, (1023,)), (8, (255, 1023))):
        for amp in amps:
            for w in TR_SIZES:
                for h in TR_SIZES:
                    for (th, tv) in TR_WORST_PAIRS:
                        if not tr_pair_allowed(w, h, th, tv):
                            continue
                        for k, l, negate in tr_aligned_set(w, h, th, tv):
                            rows.append((w, h, th, tv, k, l, int(negate), amp, bd))
    return np.array(rows, np.int32)


def tr_worst_inv_rows():
    """inverse items (w, h, th, tv, x, y, val, bd): tr_aligned_coeffs with val in {32767, -32768} at the points of tr_sample_points"""
    rows = []
    for bd in (10, 8):
        for w in TR_SIZES:
            for h in TR_SIZES:
                for (th, tv) in TR_WORST_PAIRS:
                    if not tr_pair_allowed(w, h, th, tv):
                        continue
                    for (x, y) in tr_sample_points(w, h):
                        for val in (32767, -32768):
                            rows.append((w, h, th, tv, x, y, val, bd))
    return np.array(rows, np.int32)


def chain_bound_case(bd, seed=0):
    """org / pred planes tiled with tr_aligned_block residuals (pred = 0 or max, org the other, per sign of the pattern) and the TU list
    (x, y, w, h, tr_hor, tr_ver, qp, intra, sbh) of the fused chain at low QPs: every shape of the chain's classes and of its generic path, QP in
    {0, 4, 12, 22} + 6 (bd - 8) and QP 0 itself, both slice types, sign hiding on and off, in shuffled order.  The first two 64 x 64 TUs and
    the first two TUs of every 32 x 32 cell are the DC pattern (plain, negated) at QP 0: at bit depth 10 their level meets the clip of
    Quant::quant at +32767 / -32768 (bit depth 8, residual +-255: 26111).  -> org, pred, tus, W"""
    rng = np.random.default_rng(1000 + bd + seed)
    mx = (1 << bd) - 1
    shapes = [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4),
              (64, 32), (32, 64), (16, 32), (32, 16), (64, 16), (8, 16), (16, 8), (4, 16), (4, 64), (64, 4), (16, 4), (4, 8), (8, 4), (2, 8), (8, 2), (2, 2),
              (16, 64), (32, 8), (2, 32), (8, 32), (32, 4), (4, 32), (64, 8), (8, 64)]
    qps = sorted({0} | {q + 6 * (bd - 8) for q in (0, 4, 12, 22)})
    W, H = 640, 384                                          # 60 cells of 64 x 64: every shape twice, the two largest squares once more
    org = np.zeros((H, W), np.int16)
    pred = np.zeros((H, W), np.int16)
    tus = []
    ci = 0
    for y0 in range(0, H, 64):
        for x0 in range(0, W, 64):
            w, h = shapes[ci % len(shapes)]
            rnd = ci // len(shapes)
            ci += 1
            n = 0
            for ty in range(0, 64, h):
                for tx in range(0, 64, w):
                    th = int(rng.integers(0, 3)) if 4 <= w <= 32 else 0
                    tv = int(rng.integers(0, 3)) if 4 <= h <= 32 else 0
                    pats = list(tr_aligned_set(w, h, th, tv))
                    k, l, negate = pats[(n + ci) % len(pats)]
                    qp, intra, sbh = int(qps[(n + ci // 3) % len(qps)]), (n >> 1) & 1, (n + ci) & 1
                    if w == h and w >= 32 and (n < 2 if w == 32 else rnd < 2):
                        th = tv = k = l = 0
                        qp, negate = 0, bool(n & 1 if w == 32 else rnd & 1)
                    b = tr_aligned_block(w, h, th, tv, k, l, mx, negate).astype(np.int32)
                    org[y0 + ty:y0 + ty + h, x0 + tx:x0 + tx + w] = np.where(b > 0, mx, 0)
                    pred[y0 + ty:y0 + ty + h, x0 + tx:x0 + tx + w] = np.where(b > 0, 0, mx)
                    tus.append((x0 + tx, y0 + ty, w, h, th, tv, qp, intra, sbh))
                    n += 1
    order = rng.permutation(len(tus))
    return org, pred, [tus[i] for i in order], W


SAO_ONE_CATEGORY_KINDS = ("org_max", "rec_max", "stripes")


def sao_one_category_planes(kind, w, h, bd):
    """(org, rec) with |org - rec| at the full range in every sample: constant planes (max, 0) / (0, max) -- every sample in category 2 of
    every EO class -- and (max, rec = vertical stripes of period 2 in {0, 1}), which moves everything into the categories 0 and 4 of the
    horizontal and the diagonal classes"""
    mx = (1 << bd) - 1
    org = np.full((h, w), mx if kind != "rec_max" else 0, np.int16)
    rec = np.full((h, w), mx if kind == "rec_max" else 0, np.int16)
    if kind == "stripes":
        rec[:, 1::2] = 1
    return org, rec


ALF_WORST_KINDS = (0, 64, 128, 896, 960, "max", "checker")


def alf_worst_planes(kind, w, h, bd):
    """(org, rec): rec constant at `kind` (64 and 128 make the low limb of a tap-pair sum or of the centre sample -128), org at the opposite
    extreme; 'checker': rec a checkerboard of {0, max}, org its complement"""
    mx = (1 << bd) - 1
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        rec = (((xx + yy) & 1) * mx).astype(np.int16)
        return (mx - rec).astype(np.int16), rec
    v = mx if kind == "max" else min(int(kind), mx)
    rec = np.full((h, w), v, np.int16)
    org = np.full((h, w), 0 if v > mx // 2 else mx, np.int16)
    return org, rec


# ---- inputs at the bounds of the integer searches' packed keys and of the block distortions' sums -------------------------
# kind -> (org, the two reference levels; the second one gives the larger |org - ref|)
SEARCH_BOUND_KINDS = {"bipred_hi": (2046, (1, 0)), "bipred_lo": (-1023, (1022, 1023)), "int16_hi": (32767, (1, 0)), "int16_lo": (-32768, (1022, 1023))}
# 64 x 64 samples of the larger |d|: what every position of a 64x64 block of a tie=True plane costs (the searches' `<< sub_shift` gives it back)
SEARCH_BOUND_SAD64 = {"bipred_hi": 8380416, "bipred_lo": 8380416, "int16_hi": 134213632, "int16_lo": 138407936}


def search_bound_planes(kind, tie, W, H, m):
    """(org H x W, ref (H + 2 m) x (W + 2 m)): a constant original at an end of the bi-predictive (2 org - otherPred at bit depth 10) or of the int16
    range, and a reference inside bit depth 10 at the opposite end: two adjacent levels drawn per 40 x 40 patch (SADs differ between positions by
    less than one part in a thousand), or with tie=True the one level of the larger |d| (every position of every block has the same SAD)"""
    o, (near, far) = SEARCH_BOUND_KINDS[kind]
    PW, PH = W + 2 * m, H + 2 * m
    org = np.full((H, W), o, np.int16)
    if tie:
        return org, np.full((PH, PW), far, np.int16)
    rng = np.random.default_rng(4000 + sorted(SEARCH_BOUND_KINDS).index(kind))
    pick = rng.integers(0, 2, (PH // 40 + 1, PW // 40 + 1)).repeat(40, 0).repeat(40, 1)[:PH, :PW]
    return org, np.ascontiguousarray(np.where(pick, far, near).astype(np.int16))


# (lambda, pred_hor, pred_ver) at cost_scale 2: every cost equal; the realistic top; a near predictor (the bits vary over the grid: differences in
# bits 16..22 of the cost); a far predictor (59 or 61 bits per component: lambda * bits in [2^28, 2^29) at every position, the top of the 32-bit keys)
SEARCH_BOUND_MVCOSTS = [(0.0, 0, 0), (1000.0, 37, -22), (65536.5, -58, 41), (3999999.5, -(1 << 29), 1 << 29)]
# vvcgpu_tz_search_batch takes lambda < 2^20
SEARCH_BOUND_MVCOSTS_TZ = SEARCH_BOUND_MVCOSTS[:3] + [(1048575.5,) + SEARCH_BOUND_MVCOSTS[3][1:]]

DIST_BOUND_KINDS = ("const", "checker", "half")


def dist_bound_planes(kind, W, H, bd):
    """(org, cur) of one W x H block with |org - cur| = max in every sample: 'const' org = max, cur = 0 (the largest DC Hadamard coefficient);
    'checker' cur a checkerboard of {0, max}, org its inverse (the highest-frequency coefficient); 'half' +max in the left half of every row and
    -max in the right half (the mean-removed kinds subtract a zero mean from maximal differences)"""
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "const":
        cur = np.zeros((H, W), np.int16)
    elif kind == "checker":
        cur = (((xx + yy) & 1) * mx).astype(np.int16)
    elif kind == "half":
        cur = ((xx >= W // 2) * mx).astype(np.int16)
    else:
        raise ValueError(kind)
    return (mx - cur).astype(np.int16), cur


SEARCH_BIT31_MV = (-5, 10)


def search_bit31_planes(o, W, H, m, x0, y0, bw, bh):
    """(org = o everywhere, ref = 0 but 1 where the bw x bh block at (x0, y0) lies when displaced by SEARCH_BIT31_MV): the block's SAD is at most bw bh o
    and lowest, bw bh less, at that displacement; its neighbours overlap the patch of ones partly and lie between.  With bw bh o = 61 440 000 (64 x 64 x 15000, 16 x 128 x 30000) and the fourth entry of
    SEARCH_BOUND_MVCOSTS the winner's raster key (cost << 2 | candidate, 118 bits) is just below 2^31 and the key of (0, 10) -- 120 bits, the last of
    the four candidates a lane folds together with the winner -- just above: a signed 32-bit minimum inside the lane would prefer it"""
    org = np.full((H, W), o, np.int16)
    ref = np.zeros((H + 2 * m, W + 2 * m), np.int16)
    dx, dy = SEARCH_BIT31_MV
    ref[m + y0 + dy:m + y0 + dy + bh, m + x0 + dx:m + x0 + dx + bw] = 1
    return org, ref


# ---- deblocking: inputs that take every filter decision at its threshold (tests/test_deblock_census_cpu.py counts them) ------------
DBK_TC = np.array([0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40,
                                                                    42, 44, 46, 48])
DBK_BETA = np.array([0] * 16 + list(range(6, 19)) + list(range(20, 90, 2)))
DBK_QP_KINDS = ("uniform", "mid", "low", "high", "ends")


def deblock_qp_map(rng, shape, kind):
    """CU QPs of [-12, 63] (the reference's range at bit depth 10): 'uniform' over all of it; 'mid' 20..49 where tc and beta are both at work, one unit in five
    uniform; 'low' -12..8 and 'high' 50..63 (the clamps of the table indices, chroma QPs beyond the mapping table); 'ends' a third of each"""
    uni = rng.integers(-12, 64, shape)
    if kind == "uniform":
        q = uni
    elif kind == "mid":
        q = np.where(rng.random(shape) < 0.8, rng.integers(20, 50, shape), uni)
    elif kind == "low":
        q = rng.integers(-12, 9, shape)
    elif kind == "high":
        q = rng.integers(50, 64, shape)
    elif kind == "ends":
        q = np.choose(rng.integers(0, 3, shape), [rng.integers(-12, 9, shape), rng.integers(50, 64, shape), uni])
    else:
        raise ValueError(kind)
    return q.astype(np.int8)


def deblock_maps_wide(rng, w, h, qp_kind, keep_ver=1.0, keep_hor=1.0, all_set=False):
    """deblock_maps(..., 'random') -- every BS / flag combination it allows -- with the QP maps of deblock_qp_map; keep_*: the share of edge bytes that
    stay (a horizontal decision then sees samples that no vertical pass has touched); all_set: no byte is zero"""
    ev, eh, _, _ = deblock_maps(rng, w, h, "random")
    for m, keep in ((ev, keep_ver), (eh, keep_hor)):
        if all_set:
            m[(m & 3) == 0] |= 1
            m[((m >> 2) & 3) < 2] = (m[((m >> 2) & 3) < 2] & 0xF3) | 8
        m[rng.random(m.shape) >= keep] = 0
    return ev, eh, deblock_qp_map(rng, ev.shape, qp_kind), deblock_qp_map(rng, ev.shape, qp_kind)


def deblock_lattice_plane(rng, h, w, bd, step, spread, lattice=True):
    """flat in 8 x 8 blocks: a level per 32 x 32 region anywhere in 0 .. 2^bd - 1 (the margins of a narrowed clip range included), the blocks of a region
    within +-step of it.  Only lines 0 and 3 of a 4-line segment enter the luma decisions, so the samples at x % 4 in {1, 2} and y % 4 in {1, 2} -- m1, m2, m5, m6
    of lines 1 and 2, in both directions -- vary freely by +-spread: segments that pass d < beta and the strong test on their smooth lines filter rough ones.
    lattice=False (chroma, which takes no decision): every sample varies"""
    mx = (1 << bd) - 1
    by, bx = (h + 7) // 8, (w + 7) // 8
    coarse = rng.integers(0, mx + 1, ((h + 31) // 32, (w + 31) // 32)).repeat(4, 0).repeat(4, 1)[:by, :bx]
    a = np.clip(coarse + rng.integers(-step, step + 1, (by, bx)), 0, mx).repeat(8, 0).repeat(8, 1)[:h, :w]
    yy, xx = np.mgrid[0:h, 0:w]
    free = ((xx % 4 == 1) | (xx % 4 == 2)) & ((yy % 4 == 1) | (yy % 4 == 2)) if lattice else np.ones((h, w), bool)
    a = np.where(free, np.clip(a + rng.integers(-spread, spread + 1, (h, w)), 0, mx), a)
    return np.ascontiguousarray(a.astype(np.int16))


def _dbk_weak_delta(s):
    return (6 * s + 8) >> 4                 # delta of the weak filter across a step s between two flat sides


def _dbk_step_for(t):
    """the smallest |s| whose weak-filter delta is t (t may be negative)"""
    s = np.arange(0, 6000) * (1 if t >= 0 else -1)
    hit = np.nonzero(_dbk_weak_delta(s) == t)[0]
    return int(s[hit[0]]) if hit.size else None


DBK_TARGETS = ("d_beta", "d_beta_m1", "ds_thr", "ds_thr_m1", "dd_thr", "dd_thr_m1", "dm_thr", "dm_thr_m1", "side", "side_m1", "delta")


def _dbk_solve_segment(rng, target, tc, beta, mx):
    """4 lines x 8 samples (m0 .. m7) across one edge, relative to an arbitrary level, that put `target` on its threshold; None where tc / beta leave no room.
    The sides are flat (m1 = m2 = m3 = P, m4 = m5 = m6 = Q), then: m1 = P + k gives dp = k, m6 = Q + k gives dq = k, m0 / m7 give the ds term, Q - P the
    dm term and the weak filter's delta"""
    r = np.zeros((4, 8), np.int64)
    sg = lambda: int(rng.choice((-1, 1)))
    dmThr = (5 * tc + 1) >> 1

    def step(s, lines=range(4)):
        for i in lines:
            r[i, 4:] += s

    def split(v, n):
        cut = np.sort(rng.integers(0, v + 1, n - 1))
        return np.diff(np.concatenate(([0], cut, [v])))

    small = int(rng.integers(0, dmThr)) * sg() if dmThr > 0 else 0              # a step that passes the dm term
    a, b = (0, 3) if rng.random() < 0.5 else (3, 0)                             # the line that carries the event, and the other decision line
    if target in ("d_beta", "d_beta_m1"):
        v = beta - (target == "d_beta_m1")
        if v < 0:
            return None
        k = split(v, 4)
        r[0, 1] += k[0] * sg(); r[0, 6] += k[1] * sg(); r[3, 1] += k[2] * sg(); r[3, 6] += k[3] * sg()
        step(int(rng.integers(2, 3 + 2 * tc)) * sg())
    elif target in ("ds_thr", "ds_thr_m1"):
        v = (beta >> 3) - (target == "ds_thr_m1")
        if v < 0 or (beta >> 3) < 1 or dmThr < 1:
            return None
        k = split(v, 2)
        r[a, 0] += k[0] * sg(); r[a, 7] += k[1] * sg()
        k = split(int(rng.integers(0, beta >> 3)), 2)
        r[b, 0] += k[0] * sg(); r[b, 7] += k[1] * sg()
        step(small)
    elif target in ("dd_thr", "dd_thr_m1"):
        v = (beta >> 2) - (target == "dd_thr_m1")
        if v < 0 or v & 1 or (beta >> 3) < 1 or dmThr < 1:
            return None
        k = split(v >> 1, 2)
        r[a, 1] += k[0] * sg(); r[a, 6] += k[1] * sg()
        k = split(int(rng.integers(0, ((beta >> 2) + 1) >> 1)), 2)
        r[b, 1] += k[0] * sg(); r[b, 6] += k[1] * sg()
        step(small)
    elif target in ("dm_thr", "dm_thr_m1"):
        v = dmThr - (target == "dm_thr_m1")
        if v < 0 or dmThr < 1 or (beta >> 3) < 1:
            return None
        step(v * sg())
        if rng.random() < 0.5:                                                  # the other decision line well inside
            step(-int(np.sign(r[0, 4])) * int(rng.integers(0, v + 1)), [b])
    elif target in ("side", "side_m1"):
        side = (beta + (beta >> 1)) >> 3
        v = side - (target == "side_m1")
        if v < 0 or tc < 1:
            return None
        k = split(v, 2)
        j = 1 if rng.random() < 0.5 else 6
        r[0, j] += k[0] * sg(); r[3, j] += k[1] * sg()
        r[a, 0 if rng.random() < 0.5 else 7] += ((beta >> 3) + 1 + int(rng.integers(0, 4))) * sg()      # ds fails: the weak filter
        step(int(rng.integers(2, 3 + 2 * tc)) * sg())
    elif target == "delta":
        if beta < 1:
            return None
        r[a, 0 if rng.random() < 0.5 else 7] += ((beta >> 3) + 1 + int(rng.integers(0, 4))) * sg()
        for i in range(4):                                                      # every line its own step: |delta| at 10 tc - 1, 10 tc, 10 tc + 1, tc, tc + 1
            t = int(rng.choice((10 * tc - 1, 10 * tc, 10 * tc + 1, tc, tc + 1))) * sg()
            s = _dbk_step_for(t)
            if s is None or abs(s) > mx:
                s = _dbk_step_for((tc + 1) * sg())
            step(s, [i])
            r[i] -= int(rng.integers(0, 2)) * s                                 # P or Q stays at the common level
    else:
        raise ValueError(target)
    if rng.random() < 0.5:                                                      # rough lines 1 and 2 behind smooth decision lines
        spread = int(rng.choice((2, 8, 40, 200)))
        r[1:3, [1, 2, 5, 6]] += rng.integers(-spread, spread + 1, (2, 4))
    return r if r.max() - r.min() <= mx else None


def deblock_threshold_plane(rng, h, w, ev, qpl, cfg):
    """luma plane for VERTICAL edges alone (the caller zeroes edge_hor, or transposes everything): each 4-row segment of each edge of the 8-sample grid owns
    samples x - 4 .. x + 3, draws one of DBK_TARGETS and gets the samples that put it there for the tc and beta its map bytes and cfg give (the tables
    above restate LoopFilter.cpp:66-80)"""
    bd = cfg["bd_luma"]
    mx, scale = (1 << bd) - 1, 1 << (bd - 8)
    Y = deblock_lattice_plane(rng, h, w, bd, 2 * scale, 4 * scale).astype(np.int64)
    for x in range(8, w, 8):
        for uy in range(h // 4):
            e = int(ev[uy, x // 4])
            bs = e & 3
            if not bs:
                continue
            qp = (int(qpl[uy, x // 4 - 1]) + int(qpl[uy, x // 4]) + 1) >> 1
            tc = int(DBK_TC[min(max(qp + 2 * (bs - 1) + 2 * cfg["tc_off"], 0), 65)]) * scale
            beta = int(DBK_BETA[min(max(qp + 2 * cfg["beta_off"], 0), 63)]) * scale
            r = _dbk_solve_segment(rng, DBK_TARGETS[int(rng.integers(0, len(DBK_TARGETS)))], tc, beta, mx)
            if r is None:
                continue
            Y[4 * uy:4 * uy + 4, x - 4:x + 4] = r + int(rng.integers(-r.min(), mx - r.max() + 1))
    return np.ascontiguousarray(Y.astype(np.int16))


def deblock_transpose(c):
    """the case mirrored at the diagonal: vertical edges become horizontal ones"""
    t = dict(c, w=c["h"], h=c["w"], name=c["name"] + "-T")
    for k in ("Y", "Cb", "Cr", "qpl", "qpc"):
        t[k] = np.ascontiguousarray(c[k].T)
    t["ev"], t["eh"] = np.ascontiguousarray(c["eh"].T), np.ascontiguousarray(c["ev"].T)
    return t


# bit depths (luma, chroma), beta / tc offsets (div 2), Cb / Cr QP offsets, narrowed clip range: 8, 9, 10 bit, one mixed pair, the offsets' corners
DBK_CFGS = [(10, 10, 0, 0, 0, 0, False), (8, 8, 6, -6, 12, -12, True), (9, 9, -6, 6, -12, 12, False), (10, 8, 2, -1, 12, 12, True),
            (8, 8, -6, -6, -12, -12, False), (10, 10, 6, 6, 3, -5, True), (9, 9, 0, 3, 12, 12, True), (10, 10, -3, 1, -12, -12, False)]
# a narrowed clip range, different per component, in units of 2^(bd - 8)
DBK_NARROW = ((16, 235), (9, 247), (27, 224))


def deblock_cfg_dict(bdl, bdc, beta_off, tc_off, cb_off, cr_off, narrow):
    bds = (bdl, bdc, bdc)
    lo = [DBK_NARROW[i][0] << (bds[i] - 8) if narrow else 0 for i in range(3)]
    hi = [(DBK_NARROW[i][1] << (bds[i] - 8)) + (3 if bds[i] > 8 else 0) if narrow else (1 << bds[i]) - 1 for i in range(3)]
    return dict(bd_luma=bdl, bd_chroma=bdc, beta_off=beta_off, tc_off=tc_off, cb_off=cb_off, cr_off=cr_off, clp_min=lo, clp_max=hi)


def deblock_cfg_struct(cfg):
    import ctypes as C
    from vvcsoftware_vtm_amd.abi import DeblockCfg
    return DeblockCfg(cfg["bd_luma"], cfg["bd_chroma"], cfg["beta_off"], cfg["tc_off"], cfg["cb_off"], cfg["cr_off"],
                      (C.c_int32 * 3)(*cfg["clp_min"]), (C.c_int32 * 3)(*cfg["clp_max"]))


def _dbk_chroma(rng, c, spread):
    bd, sc = c["cfg"]["bd_chroma"], 1 << (c["cfg"]["bd_chroma"] - 8)
    for k in ("Cb", "Cr"):
        c[k] = deblock_lattice_plane(rng, c["h"] // 2, c["w"] // 2, bd, 3 * sc, spread * sc, lattice=False)


def deblock_lattice_case(seed, w, h, cfg, qp_kind, step, spread, keep_ver=1.0, all_set=False, wild=False):
    """step / spread in units of 2^(bd - 8).  wild: one sample in 30 outside the bit depth, up to +-32767: among the free samples of the lattice (they reach
    the filters of segments whose decision lines stay smooth) and anywhere"""
    rng = np.random.default_rng(seed)
    c = dict(name="lattice-%d-%dx%d" % (seed, w, h), w=w, h=h, cfg=cfg)
    sc = 1 << (cfg["bd_luma"] - 8)
    c["Y"] = deblock_lattice_plane(rng, h, w, cfg["bd_luma"], step * sc, spread * sc)
    _dbk_chroma(rng, c, min(spread, 40))
    if wild:
        c["name"] = "wild-" + c["name"]
        for k in ("Y", "Cb", "Cr"):
            a = c[k]
            yy, xx = np.mgrid[0:a.shape[0], 0:a.shape[1]]
            free = ((xx % 4 == 1) | (xx % 4 == 2)) & ((yy % 4 == 1) | (yy % 4 == 2))
            m = (rng.random(a.shape) < 0.12) & free | (rng.random(a.shape) < 0.004)
            a[m] = rng.choice(np.array([-32767, -32768, -4000, -37, -1, (1 << cfg["bd_luma"]), 3000, 20000, 32767], np.int16), int(m.sum()))
    c["ev"], c["eh"], c["qpl"], c["qpc"] = deblock_maps_wide(rng, w, h, qp_kind, keep_ver=keep_ver, all_set=all_set)
    return c


def deblock_threshold_case(seed, w, h, cfg, qp_kind, transposed):
    """vertical-only form (edge_hor all zero), or built at h x w and transposed: a horizontal decision then never depends on an earlier vertical pass"""
    rng = np.random.default_rng(seed)
    if transposed:
        w, h = h, w
    c = dict(name="threshold-%d-%dx%d" % (seed, w, h), w=w, h=h, cfg=cfg)
    c["ev"], c["eh"], c["qpl"], c["qpc"] = deblock_maps_wide(rng, w, h, qp_kind, keep_hor=0.0)
    c["Y"] = deblock_threshold_plane(rng, h, w, c["ev"], c["qpl"], cfg)
    _dbk_chroma(rng, c, 12)
    return deblock_transpose(c) if transposed else c


DBK_CONTENT_SIZES = ((136, 72), (200, 120))
DBK_SPREADS = (3, 12, 48, 255)              # of the lattice's free samples, in units of 2^(bd - 8): a few units .. the whole range
_dbk_cases = None


def deblock_census_cases():
    """the input set of tests/test_deblock_census_cpu.py and of the device tests that share it -> list of dicts (name, w, h, Y, Cb, Cr, ev, eh, qpl, qpc, cfg).
    Built once; the tests copy what they filter"""
    global _dbk_cases
    if _dbk_cases is not None:
        return _dbk_cases
    out = []
    n = 0
    for (w, h) in DBK_CONTENT_SIZES:
        for i, row in enumerate(DBK_CFGS):
            cfg = deblock_cfg_dict(*row)
            for j in range(2):
                out.append(deblock_lattice_case(7000 + n, w, h, cfg, DBK_QP_KINDS[(n + (n // 5)) % 5], step=(1, 2, 4, 9)[(i + j) % 4], spread=DBK_SPREADS[(n // 2 + j) % 4],
                                                keep_ver=(1.0, 0.3)[j]))
                n += 1
            for transposed in (False, True):
                out.append(deblock_threshold_case(7000 + n, w, h, cfg, ("mid", "uniform", "mid", "high", "mid")[n % 5], transposed))
                n += 1
    # 8 x 8 has no interior edge; 16 x 8 / 8 x 16 one; 520 x 24: 66 blocks per block row, two wavefronts, the second one with two lanes
    for k, (w, h) in enumerate(((8, 8), (16, 8), (8, 16), (520, 24), (520, 24))):
        out.append(deblock_lattice_case(7900 + k, w, h, deblock_cfg_dict(*DBK_CFGS[(0, 3, 1, 5, 2)[k]]), "mid", 2, 48, all_set=w < 100))
    out.append(deblock_lattice_case(7950, 136, 72, deblock_cfg_dict(*DBK_CFGS[0]), "mid", 2, 12, wild=True))
    out.append(deblock_lattice_case(7951, 200, 120, deblock_cfg_dict(*DBK_CFGS[3]), "mid", 3, 48, wild=True))
    _dbk_cases = out
    return out
