"""The baseline JPEG round trip (save with quality Q and subsampling S, load again) restated in numpy from the rule in the header comment
of rcot_amd/csrc/jpeg.hip: colour conversion, chroma subsampling, the "islow" integer DCT, quantisation and their inverses — entropy
coding is lossless, so no bitstream is made.  Everything is computed in int64 and every intermediate is ASSERTED to fit 32 bits (the
kernel works in 32-bit integers).  ``JpegDouble`` is the CPU double of the backend for the folder loader."""
import numpy as np
import torch

from host_double import TorchDouble
from rcot_amd.jpeg import quant_tables

I64 = np.int64


def fits32(*arrays):
    for a in arrays:
        a = np.asarray(a)
        if a.size:
            assert -(1 << 31) <= int(a.min()) and int(a.max()) < (1 << 31), "an intermediate leaves 32 bits"
    return arrays[0] if len(arrays) == 1 else arrays


def FIX(x):
    return int(x * 65536 + 0.5)


def D(x, n):
    """descale: add half, arithmetic shift right by n"""
    return fits32(x + (1 << (n - 1))) >> n


# ------------------------------------------------------------------ colour
def rgb_to_ycc(img):
    r, g, b = (img[..., c].astype(I64) for c in range(3))
    y = fits32(FIX(.299) * r + FIX(.587) * g + FIX(.114) * b + 32768) >> 16
    cb = fits32(-FIX(.16874) * r - FIX(.33126) * g + FIX(.5) * b + (128 << 16) + 32767) >> 16
    cr = fits32(FIX(.5) * r - FIX(.41869) * g - FIX(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def ycc_to_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + (fits32(FIX(1.402) * cr + 32768) >> 16)
    b = y + (fits32(FIX(1.772) * cb + 32768) >> 16)
    g = y + (fits32(-FIX(.34414) * cb + 32768 - FIX(.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def pad_edge(p, h, w):
    """replicate the last row / column of a plane up to h x w"""
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def up(n, m):
    return -(-n // m) * m


# ------------------------------------------------------------------ the two 8-point transforms (12 constants, 13 bits)
C_0_298, C_0_390, C_0_541, C_0_765, C_0_899, C_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
C_1_501, C_1_847, C_1_961, C_2_053, C_2_562, C_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def fdct_1d(d, first):
    """d: list of 8 int64 arrays.  first: the row pass (DC terms << 2, others D(., 11)); else the column pass (D(., 2) and D(., 15))"""
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = fits32((t10 + t11) << 2) if first else D(t10 + t11, 2)
    o[4] = fits32((t10 - t11) << 2) if first else D(t10 - t11, 2)
    z1 = fits32((t12 + t13) * C_0_541)
    o[2] = D(z1 + fits32(t13 * C_0_765), n)
    o[6] = D(z1 - fits32(t12 * C_1_847), n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = fits32((z3 + z4) * C_1_175)
    t4, t5, t6, t7 = fits32(t4 * C_0_298, t5 * C_2_053, t6 * C_3_072, t7 * C_1_501)
    z1, z2, z3, z4 = fits32(-z1 * C_0_899, -z2 * C_2_562, -z3 * C_1_961, -z4 * C_0_390)
    z3, z4 = z3 + z5, z4 + z5
    o[7], o[5], o[3], o[1] = D(t4 + z1 + z3, n), D(t5 + z2 + z4, n), D(t6 + z2 + z3, n), D(t7 + z1 + z4, n)
    return o


def idct_1d(c, n):
    """c: list of 8 int64 arrays -> 8 outputs, each D(., n) (11 for the column pass, 18 for the row pass)"""
    z1 = fits32((c[2] + c[6]) * C_0_541)
    t2, t3 = z1 - fits32(c[6] * C_1_847), z1 + fits32(c[2] * C_0_765)
    t0, t1 = fits32((c[0] + c[4]) << 13, (c[0] - c[4]) << 13)
    t10, t13, t11, t12 = fits32(t0 + t3, t0 - t3, t1 + t2, t1 - t2)
    a0, a1, a2, a3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = fits32((z3 + z4) * C_1_175)
    a0, a1, a2, a3 = fits32(a0 * C_0_298, a1 * C_2_053, a2 * C_3_072, a3 * C_1_501)
    z1, z2, z3, z4 = fits32(-z1 * C_0_899, -z2 * C_2_562, -z3 * C_1_961, -z4 * C_0_390)
    z3, z4 = z3 + z5, z4 + z5
    a0, a1, a2, a3 = fits32(a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4)
    return [D(t10 + a3, n), D(t11 + a2, n), D(t12 + a1, n), D(t13 + a0, n), D(t13 - a0, n), D(t12 - a1, n), D(t11 - a2, n), D(t10 - a3, n)]


def block_roundtrip(plane, q):
    """plane int64 [8 m, 8 n] of samples 0..255, q int64 [8, 8] -> the decoded plane, 0..255"""
    h, w = plane.shape
    b = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)                 # [by, bx, row, column]
    rows = np.stack(fdct_1d([b[..., k] for k in range(8)], True), axis=-1)               # along the row: the last axis
    coef = np.stack(fdct_1d([rows[..., k, :] for k in range(8)], False), axis=-2)        # then along the column
    d = 8 * q
    n = fits32(np.abs(coef) + (d >> 1))
    assert int(n.max()) < (1 << 17)                                                      # the kernel's reciprocal is exact below 2^21
    deq = fits32(np.sign(coef) * (n // d) * q)
    cols = np.stack(idct_1d([deq[..., k, :] for k in range(8)], 11), axis=-2)
    out = np.stack(idct_1d([cols[..., k] for k in range(8)], 18), axis=-1)
    out = np.clip(out + 128, 0, 255)
    return out.transpose(0, 2, 1, 3).reshape(h, w)


# ------------------------------------------------------------------ chroma subsampling
def downsample_420(c, H, W):
    """full-resolution chroma [H, W] -> the plane the encoder transforms: [multiple of 8, multiple of 8]"""
    c = pad_edge(c, up(H, 2), up(W, 16))
    bias = np.where(np.arange(c.shape[1] // 2) % 2 == 0, 1, 2)[None, :]
    s = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
    return pad_edge(s, up(s.shape[0], 8), s.shape[1])                                     # the DOWNSAMPLED plane's last row


def upsample_420(c, H, W):
    """decoded chroma, cropped to ceil(H / 2) x ceil(W / 2) -> [H, W] by the triangle filter"""
    hc, wc = (H + 1) // 2, (W + 1) // 2
    assert wc > 2
    c = c[:hc, :wc]
    above, below = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    v = np.empty((2 * hc, wc), dtype=I64)
    v[0::2], v[1::2] = 3 * c + above, 3 * c + below
    last, nxt = np.concatenate([v[:, :1], v[:, :-1]], axis=1), np.concatenate([v[:, 1:], v[:, -1:]], axis=1)
    o = np.empty((2 * hc, 2 * wc), dtype=I64)
    o[:, 0::2], o[:, 1::2] = (3 * v + last + 8) >> 4, (3 * v + nxt + 7) >> 4              # (the end columns: 3 v + v = 4 v)
    return o[:H, :W]


def roundtrip_np(img, quality, subsampling=2):
    """uint8 [H, W, 3] -> uint8 [H, W, 3]: what ``Image.open`` gives for the image saved as a baseline JPEG"""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and subsampling in (0, 2)
    H, W = img.shape[:2]
    ql, qc = (np.asarray(t, dtype=I64).reshape(8, 8) for t in quant_tables(quality))
    y, cb, cr = rgb_to_ycc(img)
    if subsampling == 0:
        hp, wp = up(H, 8), up(W, 8)
        y, cb, cr = (block_roundtrip(pad_edge(p, hp, wp), q)[:H, :W] for p, q in ((y, ql), (cb, qc), (cr, qc)))
    else:
        y = block_roundtrip(pad_edge(y, up(H, 16), up(W, 16)), ql)[:H, :W]
        cb, cr = (upsample_420(block_roundtrip(downsample_420(p, H, W), qc), H, W) for p in (cb, cr))
    return ycc_to_rgb(y, cb, cr)


def pil_roundtrip(img, quality, subsampling=2):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=quality, subsampling=subsampling)
    return np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))


class JpegDouble(TorchDouble):
    """``TorchDouble`` with the method ``rcot_amd.jpeg`` calls, restated on the CPU, and the cached loader's one-launch batch as a loop
    over ``patch_prep``; ``roundtrips`` counts the whole-image degradations"""

    def __init__(self, dtype=torch.float32):
        super().__init__(dtype)
        self.roundtrips = 0

    def patch_prep_batch(self, rows, P, deg_out, clean_out):
        from rcot_amd.ops import check_patch_rows
        check_patch_rows(rows, P, deg_out, clean_out)
        for b, (clean_img, deg_img, y0, x0, mode, sigma, seed) in enumerate(rows):
            self.patch_prep(clean_img, deg_img, y0, x0, P, mode, sigma, seed, deg_out[b], clean_out[b])

    def jpeg_roundtrip(self, img, quality, subsampling=2, out=None):
        self.roundtrips += 1
        r = torch.from_numpy(roundtrip_np(img.numpy(), int(quality), int(subsampling)))
        if out is not None:
            out.copy_(r)
            return out
        return r
