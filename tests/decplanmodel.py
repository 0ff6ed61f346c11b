"""Python model of the batch decoder's pass arithmetic (sla_amd/csrc/sla_dec_plan.c: slai_dec_file_cmp, slai_dec_cut,
slai_dec_layout, slai_dec_pick_wide, slai_dec_wide_capacity), written from the rules and not from the C:

  * files are ordered with the `alone` ones last, then by the launch key (C, bps, ms, order, ntaps, lms, lshift), then by item;
  * a pass is a run of files with one launch key; a file costs (extent + 64) * C sample-channels and bytes + 4 bytes; the first
    file of a pass is always admitted, the next one only while neither sum exceeds its cap; `alone` files enter no pass;
  * in a pass every file's bytes start at the next multiple of 4, its plane region at the next multiple of 64 samples;
  * the files of at least `threshold` bytes (0: none) go wide, the 8 longest of them, longest first, ties in item order.

The seeded batches (batches(), one 32-bit linear congruential stream) are the ones tests/tools/dec_plan_check.c draws and the
ones tests/golden/dec_pass_plan.json was recorded on."""
ALIGN = 64
WIDE_MAX = 8
KEY = ("C", "bps", "ms", "order", "ntaps", "lms", "lshift")
M64 = (1 << 64) - 1


class File(dict):
    """item, C, total, bps, lshift, order, ntaps, lms, ms, bytes, nb, extent, alone"""
    __getattr__ = dict.__getitem__


def key(f):
    return tuple(f[k] for k in KEY)


def order(files):
    return sorted(files, key=lambda f: (f.alone,) + key(f) + (f.item,))


def passes(files, cap_samples, cap_bytes):
    """[(start, end)] over `files` (ordered): the passes"""
    out, n = [], sum(1 for f in files if not f.alone)
    p0 = 0
    while p0 < n:
        smp = byt = 0
        p1 = p0
        while p1 < n and key(files[p1]) == key(files[p0]):
            s1, b1 = (files[p1].extent + ALIGN) * files[p1].C, files[p1].bytes + 4
            if p1 > p0 and (smp + s1 > cap_samples or byt + b1 > cap_bytes):
                break
            smp, byt, p1 = smp + s1, byt + b1, p1 + 1
        out.append((p0, p1))
        p0 = p1
    return out


def layout(files):
    """([(img_off, plane_off)], img_bytes, span, nb) of one pass; span is 0 when no file has a sample"""
    offs, img, span = [], 0, 0
    for f in files:
        offs.append((img, span))
        img += -(-f.bytes // 4) * 4
        span += -(-f.extent // ALIGN) * ALIGN
    return offs, img, span, sum(f.nb for f in files)


def pick_wide(files, threshold):
    """indices into `files`, longest first"""
    if threshold == 0:
        return []
    cand = [i for i, f in enumerate(files) if f.bytes >= threshold]
    return sorted(cand, key=lambda i: (-files[i].bytes, files[i].item))[:WIDE_MAX]


def wide_capacity(option, size):
    return option if option else max(1 << 16, size // 256)


def layout_sum(files, cuts):
    """the fixture's digest of every pass's layout (the span as the decoder takes it: 1 when 0)"""
    h = 0
    for a, b in cuts:
        offs, img, span, nb = layout(files[a:b])
        for io, po in offs:
            h = (h * 1000003 + io) & M64
            h = (h * 1000003 + po) & M64
        for v in (img, span or 1, nb):
            h = (h * 1000003 + v) & M64
    return h


class Rng:
    def __init__(self, state=20261):
        self.state = state

    def __call__(self, n):
        self.state = (self.state * 1664525 + 1013904223) & 0xFFFFFFFF
        return (self.state >> 8) % n


def batches(count):
    """[(files in item order, cap_samples, cap_bytes, threshold)]"""
    rnd, out = Rng(), []
    for _ in range(count):
        nf = 1 + rnd(40)
        cap_s = 20000 + rnd(400000)
        cap_b = 2000 + rnd(40000)
        thr = 0 if rnd(4) == 0 else 1 + rnd(6000)
        fm = []
        for _ in range(1 + rnd(3)):
            C = 1 + rnd(2); bps = 16 + 8 * rnd(2); ms = rnd(2); order_ = 8 << rnd(2); ntaps = rnd(2); lms = 4 << rnd(2); lshift = rnd(2)
            fm.append(dict(C=C, bps=bps, ms=ms, order=order_, ntaps=ntaps, lms=lms, lshift=lshift))
        files = []
        for i in range(nf):
            f = File(fm[rnd(len(fm))], item=i)
            f["total"] = rnd(100000)
            f["extent"] = 0 if rnd(8) == 0 else rnd(20000)
            f["bytes"] = 0 if rnd(8) == 0 else ((1000, 2000, 5999)[rnd(3)] if rnd(5) == 0 else rnd(6000))
            f["nb"] = rnd(50)
            f["alone"] = int(rnd(10) == 0)
            files.append(f)
        out.append((files, cap_s, cap_b, thr))
    return out
