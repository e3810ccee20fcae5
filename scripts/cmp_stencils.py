"""Outputs of the six depthwise-3x3 entry points (csrc/stencil.hip) of two builds of the library, on seeded inputs at shapes that
together reach every instantiation the dispatchers can choose.

    RCOT_LIB=<librcot_hip.so> python scripts/cmp_stencils.py dump <file>      # one process per dump, two per build
    python scripts/cmp_stencils.py cmp <parent0> <parent1> <this0> <this1>    # the first two dumps are the parent's

dump keeps, per call, the sha256 of the bytes of y / g / dd / dp / dx (equal digests = torch.equal), the weight gradient dwg itself
(zero before the call), its magnitude sum  mag = wgrad(|dd|, |p|)  (an upper bound of the sum of the magnitudes of the partial sums
that reach one address) and the instantiation: rcot_last_kernel where the dispatcher notes it, else the ladder restated here.
cmp: digests equal in all dumps; dwg equal when at most two partial sums reach an address (a two-term float sum commutes), else
the worst |a - b| / mag between any two dumps at most the worst between the parent's own two plus (contributions - 1) * 2^-23."""
import ctypes
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def ladder(planes, H, W, threshold):
    """strip_plan of csrc/stencil.hip: (G, RS, lanes combined before the atomics); G = 0: not fused"""
    cols = planes * (W // 4)
    rs = next((r for r in (16, 8) if cols * -(-H // r) >= threshold), 4)
    tpp = -(-H // rs) * (W // 4)
    if tpp % 256 == 0:
        return 256, rs, 256, tpp
    if tpp % 64 == 0:
        return 64, rs, 64, tpp
    if tpp < 64 and tpp & (tpp - 1) == 0:
        return 1, rs, tpp, tpp
    return 0, rs, 0, tpp


def nb_ok(W):
    return W % 4 == 0 and 1 <= W // 4 <= 64 and 64 % (W // 4) == 0


def wgrad_name(H, W):
    """the instantiation rcot_dwconv3x3_wgrad chooses"""
    nb4 = (H // 4) * (W // 4)
    return f"dwconv_wgrad_kernel<{16 if nb4 <= 16 else 64 if nb4 <= 64 else 256}>"


DWCONV = [(2, 144, 16, 16), (1, 288, 32, 64), (2, 1152, 8, 8), (1, 48, 128, 128), (1, 6, 256, 256), (2, 12, 64, 64), (1, 5, 64, 256),
          (2, 3, 20, 16), (2, 21, 16, 24), (1, 3, 8, 512), (2, 3, 5, 6), (1, 2, 10, 12), (1, 5, 7, 9)]
GATE_FWD = [(2, 127, 16, 16), (1, 255, 32, 32), (2, 1021, 8, 8), (1, 5, 128, 128), (1, 3, 256, 256), (2, 9, 64, 64), (1, 4, 64, 256),
            (2, 3, 20, 16), (2, 11, 16, 24), (2, 3, 5, 6), (1, 2, 10, 12), (1, 5, 7, 9)]
DWCONV_BWD = [(1, 9, 128, 128), (2, 18, 64, 64), (2, 144, 16, 16), (1, 288, 32, 64), (2, 1152, 8, 8), (2, 21, 16, 24), (3, 5, 4, 4),
              (1, 6, 256, 256), (1, 4, 64, 256), (2, 3, 20, 16), (1, 3, 24, 128),
              (2, 782, 128, 128), (1, 2084, 504, 24), (1, 1563, 128, 64), (1, 3126, 64, 64),           # the tall-strip kernel tests
              (1, 6250, 24, 128), (2, 25000, 16, 16), (2, 50000, 16, 16),                              # <64,16,t> <1,8,t> <1,16,t>
              (1, 3, 8, 512), (1, 3, 4, 512), (1, 1563, 16, 512), (1, 1563, 32, 512), (1, 1100, 24, 512)]  # <256,4,f> <64,4,f> <256,8,f> <256,16,f> <64,8,f>
GATE_BWD_DW = [(1, 5, 128, 128), (2, 9, 64, 64), (2, 31, 32, 32), (2, 127, 16, 16), (3, 37, 8, 8), (2, 11, 16, 24), (1, 3, 32, 64),
               (2, 782, 128, 128), (1, 1563, 128, 64), (1, 6250, 24, 128),                             # the tall-strip kernel tests
               (1, 3126, 64, 64), (2, 25000, 16, 16), (2, 50000, 16, 16)]                              # <64,8> <1,8> <1,16>
GATE_BWD_PLAIN = [(2, 127, 16, 16), (1, 4, 64, 256), (2, 3, 20, 16), (1, 1563, 128, 64), (2, 782, 128, 128)]   # <0,4> <0,8> <0,16>
GDFN_BWD = [(1, 5, 128, 128), (2, 9, 64, 64), (2, 31, 32, 32), (2, 127, 16, 16), (3, 37, 8, 8), (2, 11, 16, 24), (1, 3, 32, 64),
            (2, 7, 8, 40), (1, 4, 64, 256), (2, 3, 20, 16),
            (2, 391, 128, 128), (1, 3125, 24, 128), (1, 1563, 64, 64), (2, 12500, 12, 16),             # the tall-strip kernel tests
            (1, 782, 128, 64), (2, 25000, 16, 16)]                                                     # <256,8> <1,16>


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def dump(path):
    from rcot_amd.ops import HipBackend
    be = HipBackend()

    def last():
        buf = ctypes.create_string_buffer(192)
        be.L.rcot_last_kernel(buf, 192)
        return buf.value.decode()

    def rnd(seed, *shape, scale=1.0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        return torch.randn(*shape, device="cuda", generator=g) * scale

    def mag(dd, p):
        m = torch.zeros(p.shape[1], 9, device="cuda")
        be.dwconv3x3_wgrad(dd.abs(), p.abs(), m)
        return m.cpu()

    out = {}
    for (B, C, H, W) in DWCONV:
        x, w, dy = rnd(1, B, C, H, W), rnd(2, C, 9), rnd(3, B, C, H, W)
        y, yf, dw = torch.empty_like(x), torch.empty_like(x), torch.zeros(C, 9, device="cuda")
        be.dwconv3x3(x, w, y)
        k = last() if H % 4 == 0 and W % 4 == 0 else "dwconv_any_kernel"
        rec = {"y": digest(y), "kernel": k}
        if H % 4 == 0 and W % 4 == 0:
            be.dwconv3x3(x, w, yf, flip=True)
            rec.update(y_flip=digest(yf), kernel_flip=last())
            be.dwconv3x3_wgrad(dy, x, dw)
            rec.update(dwg=dw.cpu(), mag=mag(dy, x), contributions=B, kernel_wgrad=wgrad_name(H, W))
        out[("dwconv3x3", B, C, H, W)] = rec
    for (B, hid, H, W) in GATE_FWD:
        p, w = rnd(1, B, 2 * hid, H, W), rnd(2, 2 * hid, 9, scale=0.5)
        g = torch.empty(B, hid, H, W, device="cuda")
        be.gdfn_gate_fwd(p, w, g)
        k = f"gate_fwd_kernel<{str(nb_ok(W)).lower()}>" if H % 4 == 0 and W % 4 == 0 else "gate_fwd_any_kernel"
        out[("gdfn_gate_fwd", B, hid, H, W)] = {"g": digest(g), "kernel": k}
    for (B, C, H, W) in DWCONV_BWD:
        dy, x, w = rnd(1, B, C, H, W), rnd(2, B, C, H, W), rnd(3, C, 9)
        dx, dw = torch.empty_like(x), torch.zeros(C, 9, device="cuda")
        be.dwconv3x3_bwd(dy, x, w, dx, dw)
        noted = last()                                              # the fall-back route's rcot_dwconv3x3 notes its kernel
        G, RS, lanes, tpp = ladder(B * C, H, W, 400000)
        k = f"dwconv_bwd_kernel<{G}, {RS}, {str(nb_ok(W)).lower()}>" if G else f"{noted} + {wgrad_name(H, W)}"
        out[("dwconv3x3_bwd", B, C, H, W)] = {"dx": digest(dx), "dwg": dw.cpu(), "mag": mag(dy, x),
                                              "contributions": B * (tpp // lanes if G else 1), "kernel": k}
    for with_dw, shapes in ((True, GATE_BWD_DW), (False, GATE_BWD_PLAIN)):
        for (B, hid, H, W) in shapes:
            p, w, dg = rnd(1, B, 2 * hid, H, W), rnd(2, 2 * hid, 9, scale=0.5), rnd(3, B, hid, H, W)
            dd, dw = torch.empty_like(p), torch.zeros(2 * hid, 9, device="cuda")
            be.gdfn_gate_bwd(p, w, dg, dd, dw=dw if with_dw else None)
            G, RS, lanes, tpp = ladder(B * hid, H, W, 400000)
            rec = {"dd": digest(dd), "kernel": f"gate_bwd_kernel<{G if with_dw else 0}, {RS}>"}
            if with_dw:
                rec.update(dwg=dw.cpu(), mag=mag(dd, p), contributions=B * (tpp // lanes if G else 1))
                if not G:
                    rec["kernel"] += " + " + wgrad_name(H, W)
            out[("gdfn_gate_bwd" + ("+dw" if with_dw else ""), B, hid, H, W)] = rec
    for (B, hid, H, W) in GDFN_BWD:
        p, w, dg = rnd(1, B, 2 * hid, H, W), rnd(2, 2 * hid, 9, scale=0.5), rnd(3, B, hid, H, W)
        dp, dw, dd = torch.empty_like(p), torch.zeros(2 * hid, 9, device="cuda"), torch.empty_like(p)
        be.gdfn_bwd(p, w, dg, dp, dw)
        k = last()
        G, RS, lanes, tpp = ladder(B * hid, H, W, 200000)
        fused = nb_ok(W) and G
        if fused:
            assert k == f"gdfn_bwd_kernel<{G}, {RS}>", (k, G, RS)
        else:
            G, RS, lanes, tpp = ladder(B * hid, H, W, 400000)      # the two-kernel route: gate_bwd's ladder
            k = f"gate_bwd_kernel<{G}, {RS}> + " + ("" if G else wgrad_name(H, W) + " + ") + k
        be.gdfn_gate_bwd(p, w, dg, dd)                              # dd for the magnitude sum only
        out[("gdfn_bwd", B, hid, H, W)] = {"dp": digest(dp), "dwg": dw.cpu(), "mag": mag(dd, p),
                                           "contributions": B * (tpp // lanes if G else 1), "kernel": k}
    torch.cuda.synchronize()
    torch.save(out, path)
    print(f"dumped {len(out)} calls to {path}")


def cmp(paths):
    dumps = [torch.load(p, weights_only=False) for p in paths]
    assert len(dumps) == 4, "parent0 parent1 this0 this1"
    ok_all = True
    kernels = set()
    print(f"# dumps: {' '.join(os.path.basename(p) for p in paths)} (the first two: the parent build)")
    for key in dumps[0]:
        recs = [d[key] for d in dumps]
        names = [v for k, v in recs[0].items() if k.startswith("kernel")]
        assert all([v for k, v in r.items() if k.startswith("kernel")] == names for r in recs), (key, names)
        kernels.update(n for v in names for n in v.split(" + "))
        line = []
        for f in ("y", "y_flip", "g", "dd", "dp", "dx"):
            if f in recs[0]:
                same = all(r[f] == recs[0][f] for r in recs)
                ok_all &= same
                line.append(f"{f} {'bit-equal' if same else 'DIFFERS'}")
        if "dwg" in recs[0]:
            n = recs[0]["contributions"]
            if n <= 2:
                same = all(torch.equal(r["dwg"], recs[0]["dwg"]) for r in recs)
                ok_all &= same
                line.append(f"dwg ({n} partial sums per address) {'bit-equal' if same else 'DIFFERS'}")
            else:
                m = recs[0]["mag"].double().clamp_min(1e-300)
                rel = lambda a, b: float(((a["dwg"].double() - b["dwg"].double()).abs() / m).max())
                own = rel(recs[0], recs[1])
                worst = max(rel(a, b) for a, b in itertools.combinations(recs, 2))
                bound = own + (n - 1) * 2.0 ** -23
                good = worst <= bound
                ok_all &= good
                line.append(f"dwg ({n} partial sums per address) worst |a-b|/mag any two dumps {worst:.3e}, parent's own {own:.3e}, "
                            f"bar {bound:.3e} {'ok' if good else 'OUTSIDE'}")
        print(f"{key[0]:>16} {str(key[1:]):24} {' ; '.join(line)}   [{' ; '.join(names)}]")
    print("# instantiations reached:")
    for k in sorted(kernels):
        print("#   " + k)
    print("# ALL OK" if ok_all else "# FAILED")
    return 0 if ok_all else 1


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(cmp(sys.argv[2:]))
