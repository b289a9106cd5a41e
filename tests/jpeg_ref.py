"""A numpy restatement of libjpeg's baseline encoder as the device runs it: the checker of ansel_amd/csrc/jpeg.hip.

    encode(rgb, quality, subsampling, optimize, icc=None, density=(0, 1, 1)) -> bytes of a JFIF file

rgb is an (H, W, 3) or (H, W, 4) uint8 frame (alpha ignored).  subsampling 0 / 1 / 2 is 4:4:4 / 4:2:2 / 4:2:0 (Pillow's
numbering, and DT_HIP_JPEG_*).  Every stage is the integer arithmetic of libjpeg(-turbo), vectorised over blocks:
jccolor.c rgb_ycc_convert, jcsample.c h2v1 / h2v2 downsampling with the edge expansion of jcprep.c, jfdctint.c
jpeg_fdct_islow, the jcdctmgr.c quantizer, the dummy blocks of jccoefct.c, jchuff.c (statistics, jpeg_gen_optimal_table,
encode_one_block, flush) and the marker order of jcmarker.c.  The product does not import this file.
"""
import numpy as np

# jpeg_natural_order: natural (row-major) index of zigzag position k
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# jcparam.c std_luminance_quant_tbl / std_chrominance_quant_tbl (T.81 Annex K.1), natural order
STD_QUANT = (np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]),
             np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                       47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32))

# jcparam.c std_huff_tables (T.81 Annex K.3): (bits[1..16], huffval) for DC0, AC0, DC1, AC1
STD_HUFF = (
    ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
     [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21,
      82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58,
      67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116,
      117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
      162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198,
      199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234,
      241, 242, 243, 244, 245, 246, 247, 248, 249, 250]),
    ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
     [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51,
      82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58,
      67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116,
      117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153,
      154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197,
      198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234,
      242, 243, 244, 245, 246, 247, 248, 249, 250]),
)

# Y sampling factors (h, v) per mode; Cb and Cr are 1x1
SAMPLING = ((1, 1), (2, 1), (2, 2))
ICC_CHUNK = 65519


def quant_tables(quality):
    """jpeg_set_quality(quality, force_baseline=TRUE): the two tables in natural order"""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in STD_QUANT)


def ycc(rgb):
    """jccolor.c rgb_ycc_convert (SCALEBITS 16): three int32 planes"""
    def fix(x):
        return int(x * 65536 + 0.5)
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    half = 1 << 15
    off = 128 << 16
    y = (fix(0.29900) * r + fix(0.58700) * g + fix(0.11400) * b + half) >> 16
    cb = (-fix(0.16874) * r - fix(0.33126) * g + fix(0.5) * b + off + half - 1) >> 16
    cr = (fix(0.5) * r - fix(0.41869) * g - fix(0.08131) * b + off + half - 1) >> 16
    return y, cb, cr


def _comp_samples(plane, h_s, v_s, wib, hib):
    """the (hib*8, wib*8) sample array libjpeg feeds the FDCT for one component (h_s, v_s: its downsampling ratios,
    the largest sampling factor over its own): full-resolution planes are
    edge-replicated; subsampled ones are downsampled from the replicated plane (bias 0,1 / 1,2 by output column) and
    their rows past the last downsampled row replicate it"""
    H, W = plane.shape
    if h_s == 1 and v_s == 1:
        ys = np.minimum(np.arange(hib * 8), H - 1)
        xs = np.minimum(np.arange(wib * 8), W - 1)
        return plane[ys][:, xs]
    x2 = np.arange(wib * 8)
    xa = np.minimum(2 * x2, W - 1)
    xb = np.minimum(2 * x2 + 1, W - 1)
    if v_s == 1:   # h2v1
        ys = np.minimum(np.arange(hib * 8), H - 1)
        p = plane[ys]
        return (p[:, xa] + p[:, xb] + (x2 & 1)[None, :]) >> 1
    h2 = (H + 1) // 2   # h2v2
    y2 = np.minimum(np.arange(hib * 8), h2 - 1)
    pa = plane[np.minimum(2 * y2, H - 1)]
    pb = plane[np.minimum(2 * y2 + 1, H - 1)]
    return (pa[:, xa] + pa[:, xb] + pb[:, xa] + pb[:, xb] + (1 + (x2 & 1))[None, :]) >> 2


def fdct_islow(blocks):
    """jfdctint.c jpeg_fdct_islow on (N, 8, 8) centred samples (CONST_BITS 13, PASS1_BITS 2), int64"""
    CB, PB = 13, 2
    F = dict(a=2446, b=3196, c=4433, d=6270, e=7373, f=9633, g=12299, h=15137, i=16069, j=16819, k=20995, l=25172)

    def desc(x, n):
        return (x + (1 << (n - 1))) >> n

    def one_pass(d, first):
        d = [d[..., i] for i in range(8)]
        t0, t7 = d[0] + d[7], d[0] - d[7]
        t1, t6 = d[1] + d[6], d[1] - d[6]
        t2, t5 = d[2] + d[5], d[2] - d[5]
        t3, t4 = d[3] + d[4], d[3] - d[4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        o = [None] * 8
        n = CB - PB if first else CB + PB
        if first:
            o[0], o[4] = (t10 + t11) << PB, (t10 - t11) << PB
        else:
            o[0], o[4] = desc(t10 + t11, PB), desc(t10 - t11, PB)
        z1 = (t12 + t13) * F["c"]
        o[2] = desc(z1 + t13 * F["d"], n)
        o[6] = desc(z1 - t12 * F["h"], n)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * F["f"]
        t4, t5, t6, t7 = t4 * F["a"], t5 * F["j"], t6 * F["l"], t7 * F["g"]
        z1, z2, z3, z4 = -z1 * F["e"], -z2 * F["k"], -z3 * F["i"], -z4 * F["b"]
        z3 = z3 + z5
        z4 = z4 + z5
        o[7], o[5] = desc(t4 + z1 + z3, n), desc(t5 + z2 + z4, n)
        o[3], o[1] = desc(t6 + z2 + z3, n), desc(t7 + z1 + z4, n)
        return np.stack(o, -1)

    rows = one_pass(blocks.astype(np.int64), True)
    cols = one_pass(np.swapaxes(rows, -1, -2), False)
    return np.swapaxes(cols, -1, -2)


def quantize(coef, qtbl):
    """jcdctmgr.c: divide by 8*q, rounding half away from zero; (N, 64) natural order"""
    d = (8 * qtbl.astype(np.int64))[None, :]
    a = np.abs(coef)
    qv = (a + (d >> 1)) // d
    return np.where(coef < 0, -qv, qv)


def layout(W, H, subsampling):
    """per component: (h, v, width_in_blocks, height_in_blocks); and the MCU grid (mcux, mcuy)"""
    hY, vY = SAMPLING[subsampling]
    mcux = -(-W // (8 * hY))
    mcuy = -(-H // (8 * vY))
    comps = []
    for ci in range(3):
        h, v = (hY, vY) if ci == 0 else (1, 1)
        comps.append((h, v, -(-W * h // (hY * 8)), -(-H * v // (vY * 8))))
    return comps, mcux, mcuy


def coefficients(rgb, quality, subsampling):
    """quantized coefficients in scan order: (nblocks, 64) natural order int64, and each block's table (0 luma, 1
    chroma) and component, with jccoefct.c's dummy blocks in place"""
    H, W = rgb.shape[:2]
    planes = ycc(rgb)
    qt = quant_tables(quality)
    comps, mcux, mcuy = layout(W, H, subsampling)
    hY, vY = SAMPLING[subsampling]
    per_comp = []
    for ci, (h, v, wib, hib) in enumerate(comps):
        s = _comp_samples(planes[ci], hY // h, vY // v, wib, hib) - 128
        blk = s.reshape(hib, 8, wib, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        q = quantize(fdct_islow(blk).reshape(-1, 64), qt[min(ci, 1)]).reshape(hib, wib, 64)
        # the component's block grid padded to whole MCUs: dummy blocks right (DC of the block to the left) and
        # below (DC of the rightmost block of the row above, inside the same MCU)
        full = np.zeros((mcuy * v, mcux * h, 64), np.int64)
        full[:hib, :wib] = q
        for bx in range(wib, mcux * h):
            full[:hib, bx, 0] = full[:hib, bx - 1, 0]
        for by in range(hib, mcuy * v):
            # the block row above within the MCU, its last block in each MCU
            full[by, :, 0] = np.repeat(full[by - 1, h - 1::h, 0], h)
        per_comp.append(full.reshape(mcuy, v, mcux, h, 64).transpose(0, 2, 1, 3, 4).reshape(mcuy, mcux, v * h, 64))
    coefs = np.concatenate(per_comp, axis=2).reshape(-1, 64)
    nb = [c[0] * c[1] for c in comps]
    comp = np.tile(np.repeat(np.arange(3), nb), mcux * mcuy)
    return coefs, comp


def _nbits(a):
    """bit count of |a| (0 for 0)"""
    a = np.abs(a).astype(np.int64)
    n = np.zeros(a.shape, np.int64)
    while True:
        m = a > 0
        if not m.any():
            return n
        n += m
        a >>= 1


def symbols(coefs, comp):
    """every Huffman symbol in file order: (table index 0..3 = DC0 AC0 DC1 AC1, symbol, extra bits value, extra bit
    count), as flat int64 arrays"""
    N = coefs.shape[0]
    zz = coefs[:, ZIGZAG]
    dc = zz[:, 0]
    diff = np.empty(N, np.int64)
    for ci in range(3):
        idx = np.nonzero(comp == ci)[0]
        d = dc[idx]
        diff[idx] = d - np.concatenate(([0], d[:-1]))
    tbl = np.minimum(comp, 1) * 2
    # each emitted item gets a sort key block*256 + k (k: 0 DC, 1..63 AC position of the code, +ZRLs before it, 255 EOB)
    keys, tabs, syms, vals, lens = [], [], [], [], []
    nb = _nbits(diff)
    keys.append(np.arange(N) * 512)
    tabs.append(tbl)
    syms.append(nb)
    vals.append(np.where(diff < 0, diff - 1, diff) & ((1 << nb) - 1))
    lens.append(nb)
    ac = zz[:, 1:]
    b, k = np.nonzero(ac)
    k = k + 1
    # run: zeros since the previous nonzero of the same block (or since position 1)
    prev = np.empty_like(k)
    prev[0:1] = 0
    if len(k):
        prev[1:] = np.where(b[1:] == b[:-1], k[:-1], 0)
    run = k - prev - 1
    coef = ac[b, k - 1]
    nbk = _nbits(coef)
    keys.append(b * 512 + k * 8 + 7)
    tabs.append(tbl[b] + 1)
    syms.append(((run & 15) << 4) | nbk)
    vals.append(np.where(coef < 0, coef - 1, coef) & ((1 << nbk) - 1))
    lens.append(nbk)
    nz = run >> 4
    for z in range(1, 4):   # ZRLs: at most 3 (62 zeros / 16)
        m = nz >= z
        keys.append(b[m] * 512 + k[m] * 8 + z - 4 + 3)
        tabs.append(tbl[b[m]] + 1)
        syms.append(np.full(int(m.sum()), 0xF0, np.int64))
        vals.append(np.zeros(int(m.sum()), np.int64))
        lens.append(np.zeros(int(m.sum()), np.int64))
    eob = np.nonzero(ac[:, 62] == 0)[0]
    keys.append(eob * 512 + 511)
    tabs.append(tbl[eob] + 1)
    syms.append(np.zeros(len(eob), np.int64))
    vals.append(np.zeros(len(eob), np.int64))
    lens.append(np.zeros(len(eob), np.int64))
    key = np.concatenate(keys)
    order = np.argsort(key, kind="stable")
    return tuple(np.concatenate(a)[order] for a in (tabs, syms, vals, lens))


def frequencies(tabs, syms):
    """(4, 257) int64 symbol counts per table"""
    f = np.zeros((4, 257), np.int64)
    np.add.at(f, (tabs, syms), 1)
    return f


def gen_optimal_table(freq):
    """jchuff.c jpeg_gen_optimal_table: (bits[1..16], huffval) from 257 counts (256 is the reserved pseudo-symbol)"""
    freq = [int(x) for x in freq[:256]] + [1]
    codesize = [0] * 257
    others = [-1] * 257
    while True:
        c1, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [j for L in range(1, 33) for j in range(256) if codesize[j] == L]
    return bits[1:17], vals


def code_table(bits, vals):
    """jchuff.c jpeg_make_c_derived_tbl: (code, length) per symbol 0..255"""
    code = np.zeros(256, np.int64)
    size = np.zeros(256, np.int64)
    c, p = 0, 0
    for L in range(1, 17):
        for _ in range(bits[L - 1]):
            code[vals[p]] = c
            size[vals[p]] = L
            c += 1
            p += 1
        c <<= 1
    return code, size


def entropy_bytes(tabs, syms, vals, lens, tables):
    """pack codes and extra bits MSB first, pad the last byte with 1-bits, stuff 0x00 after every 0xFF"""
    ct = [code_table(*t) for t in tables]
    code = np.zeros(len(syms), np.int64)
    size = np.zeros(len(syms), np.int64)
    for t in range(4):
        m = tabs == t
        code[m] = ct[t][0][syms[m]]
        size[m] = ct[t][1][syms[m]]
        assert (size[m] > 0).all(), "symbol without a code"
    v = (code << lens) | vals
    L = size + lens                     # <= 27 bits
    end = np.cumsum(L)
    total = int(end[-1]) if len(end) else 0
    nbytes = (total + 7) // 8
    start = end - L
    byte0 = start >> 3
    # each item placed in a 40-bit window starting at its first byte; items never share bits, so byte sums are ORs
    w = v << (40 - (start & 7) - L)
    out = np.zeros(nbytes + 5, np.int64)
    for j in range(5):
        out += np.bincount(byte0 + j, weights=((w >> (32 - 8 * j)) & 255).astype(np.float64),
                           minlength=nbytes + 5).astype(np.int64)[:nbytes + 5]
    out = out[:nbytes]
    if total & 7:
        out[-1] |= (1 << (8 - (total & 7))) - 1
    b = out.astype(np.uint8)
    ff = b == 0xFF
    res = np.repeat(b, 1 + ff)
    pos = np.cumsum(1 + ff) - 1
    res[pos[ff]] = 0
    return res.tobytes()


def _marker(m, payload):
    return bytes([0xFF, m]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def headers(W, H, quality, subsampling, tables, icc=None, density=(0, 1, 1)):
    """SOI .. SOS in jcmarker.c's order"""
    unit, xd, yd = density
    out = b"\xFF\xD8" + _marker(0xE0, b"JFIF\0" + bytes([1, 1, unit]) + xd.to_bytes(2, "big") + yd.to_bytes(2, "big")
                               + b"\0\0")
    if icc:
        n = -(-len(icc) // ICC_CHUNK)
        for i in range(n):
            out += _marker(0xE2, b"ICC_PROFILE\0" + bytes([i + 1, n]) + icc[i * ICC_CHUNK:(i + 1) * ICC_CHUNK])
    for t, qt in enumerate(quant_tables(quality)):
        out += _marker(0xDB, bytes([t]) + bytes(int(x) for x in qt[ZIGZAG]))
    hY, vY = SAMPLING[subsampling]
    out += _marker(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3])
                   + bytes([1, hY * 16 + vY, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for i, (bits, vals) in enumerate(tables):
        cls, idx = i & 1, i >> 1
        out += _marker(0xC4, bytes([cls * 16 + idx]) + bytes(bits) + bytes(vals))
    out += _marker(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(rgb, quality, subsampling, optimize, icc=None, density=(0, 1, 1)):
    rgb = np.ascontiguousarray(rgb[..., :3])
    H, W = rgb.shape[:2]
    coefs, comp = coefficients(rgb, quality, subsampling)
    tabs, syms, vals, lens = symbols(coefs, comp)
    if optimize:
        f = frequencies(tabs, syms)
        tables = [gen_optimal_table(f[t]) for t in range(4)]
    else:
        tables = [(list(b), list(v)) for b, v in STD_HUFF]
    return (headers(W, H, quality, subsampling, tables, icc, density) + entropy_bytes(tabs, syms, vals, lens, tables)
            + b"\xFF\xD9")


def pillow(rgb, quality, subsampling, optimize, icc=None, dpi=None):
    """the same frame through Pillow's libjpeg(-turbo), or None without Pillow"""
    try:
        from PIL import Image, ImageFile
    except ImportError:
        return None
    import io
    im = Image.fromarray(np.ascontiguousarray(rgb[..., :3]))
    kw = dict(quality=quality, subsampling=subsampling, optimize=bool(optimize))
    if icc:
        kw["icc_profile"] = icc
    if dpi:
        kw["dpi"] = dpi
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, rgb.shape[0] * rgb.shape[1] * 4 + (len(icc) if icc else 0) + (1 << 20))
    try:
        b = io.BytesIO()
        im.save(b, "JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return b.getvalue()


def frame(kind, w, h, seed=0):
    """the test contents: gradient+noise, zero, full, primaries checkerboard, uniform noise; (h, w, 4) uint8"""
    rng = np.random.default_rng(seed)
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        img = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x ^ y) & 255], -1)
        img = np.clip(img + rng.integers(-12, 13, img.shape), 0, 255)
    elif kind == "zero":
        img = np.zeros((h, w, 3), np.int64)
    elif kind == "full":
        img = np.full((h, w, 3), 255, np.int64)
    elif kind == "primaries":
        y, x = np.mgrid[0:h, 0:w]
        prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]])
        img = prim[((x // 3) + (y // 5) * 2) % 6]
    elif kind == "noise":
        img = rng.integers(0, 256, (h, w, 3))
    else:
        raise ValueError(kind)
    out = np.empty((h, w, 4), np.uint8)
    out[..., :3] = img
    out[..., 3] = 255
    return out
