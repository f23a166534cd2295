"""Helper of tests/test_cavlc_host.py: a plain reader of slice_data() for an I slice of I_16x16 macroblocks under CAVLC (H.264 7.3.4,
7.3.5, 7.3.5.3.2) -- mb_type, intra_chroma_pred_mode, mb_qp_delta and residual_block_cavlc -- back into the arrays of an x264hip_mb_state.
It exists to read what the reference cannot check: levels beyond what its quantiser produces, through the writer's extended escape.  The
level arithmetic is restated from the decoder's side (9.2.2.1); coeff_token, total_zeros and run_before are looked up in the data of
csrc/cavlc_tables.h, which the real-content fixtures pin."""
import os
import re

import numpy as np

from paths import ROOT


def tables():
    """{name: [values]} of csrc/cavlc_tables.h; the code tables as {(length, bits): index} per group of `group` entries."""
    text = open(os.path.join(ROOT, "x264_vs2008_amd", "csrc", "cavlc_tables.h")).read()
    raw = {m.group(1): [int(v, 0) for v in re.findall(r"0x[0-9a-fA-F]+|\d+", m.group(2))]
           for m in re.finditer(r"c_cv_(\w+)\[\d+\] = \{(?:\s*//[^\n]*)?([^}]*)\}", text)}

    def decode(vals, group):
        return [{(e & 0xff, e >> 8): i for i, e in enumerate(vals[g:g + group]) if e & 0xff} for g in range(0, len(vals), group)]
    token = []
    for c in range(5):                                   # nC class: total * 4 + trailing - 4 for total >= 1, and the code of "no coefficients"
        d = {k: (i // 4 + 1, i % 4) for k, i in decode(raw["coeff"][64 * c:64 * c + 64], 64)[0].items()}
        d[(raw["coeff0"][c] & 0xff, raw["coeff0"][c] >> 8)] = (0, 0)
        token.append(d)
    return dict(token=token, total_zeros=decode(raw["total_zeros"], 16), total_zeros_dc=decode(raw["total_zeros_dc"], 4), run_before=decode(raw["run_before"], 16))


class Bits:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def u(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | (self.d[self.pos >> 3] >> (7 - (self.pos & 7)) & 1)
            self.pos += 1
        return v

    def ue(self):
        z = 0
        while not self.u(1):
            z += 1
        return (1 << z) - 1 + self.u(z)

    def se(self):
        k = self.ue()
        return (k + 1) >> 1 if k & 1 else -(k >> 1)

    def vlc(self, table):
        n, v = 0, 0
        while True:
            v, n = (v << 1) | self.u(1), n + 1
            if (n, v) in table:
                return table[(n, v)]
            assert n < 17, "no code of the table at bit %d" % (self.pos - n)


def residual_block(b, t, n_c, max_coeff):
    """residual_block_cavlc: the max_coeff coefficients in scan order and TotalCoeff.  n_c: -1 chroma DC."""
    total, trailing = b.vlc(t["token"][4 if n_c < 0 else 0 if n_c < 2 else 1 if n_c < 4 else 2 if n_c < 8 else 3])
    out = [0] * max_coeff
    if not total:
        return out, 0
    suffix_length, level = int(total > 10 and trailing < 3), []
    for i in range(total):
        if i < trailing:
            level.append(1 - 2 * b.u(1))
            continue
        prefix = 0
        while not b.u(1):
            prefix += 1
        size = prefix - 3 if prefix >= 15 else 4 if prefix == 14 and suffix_length == 0 else suffix_length
        code = (min(15, prefix) << suffix_length) + b.u(size)
        if prefix >= 15 and suffix_length == 0:
            code += 15
        if prefix >= 16:
            code += (1 << (prefix - 3)) - 4096
        if i == trailing and trailing < 3:
            code += 2
        level.append((code + 2) >> 1 if code % 2 == 0 else (-code - 1) >> 1)
        if suffix_length == 0:
            suffix_length = 1
        if abs(level[-1]) > (3 << (suffix_length - 1)) and suffix_length < 6:
            suffix_length += 1
    zeros_left = 0
    if total < max_coeff:
        zeros_left = b.vlc((t["total_zeros_dc"] if n_c < 0 else t["total_zeros"])[total - 1])
    pos = zeros_left + total - 1                          # the highest coefficient's place; level[0] is that coefficient
    for i in range(total):
        out[pos] = level[i]
        run = 0
        if i < total - 1 and zeros_left > 0:
            run = b.vlc(t["run_before"][min(zeros_left - 1, 6)])
            zeros_left -= run
        pos -= 1 + run
    return out, total


def read_i16_slice(data, mb_w, mb_h, slice_qp):
    """slice_data() of an I slice whose macroblocks are all I_16x16 -> {i16mode, chroma_mode, qp, cbp, luma, luma_dc, chroma_dc, chroma_ac}
    as an x264hip_mb_state holds them, and the bit position behind every macroblock.  Anything else in the bytes raises."""
    t, b, n = tables(), Bits(data), mb_w * mb_h
    out = dict(i16mode=np.zeros(n, np.int8), chroma_mode=np.zeros(n, np.int8), qp=np.zeros(n, np.int8), cbp=np.zeros(n, np.int16),
               luma=np.zeros((n, 256), np.int16), luma_dc=np.zeros((n, 16), np.int16), chroma_dc=np.zeros((n, 8), np.int16), chroma_ac=np.zeros((n, 128), np.int16))
    # TotalCoeff of every 4x4 block of the picture: luma, Cb, Cr (the slice is the picture: a block is available iff it lies inside)
    tot = [np.zeros((4 * mb_h, 4 * mb_w), int), np.zeros((2 * mb_h, 2 * mb_w), int), np.zeros((2 * mb_h, 2 * mb_w), int)]

    def n_c(plane, x, y):
        a, bb = (tot[plane][y, x - 1] if x > 0 else None), (tot[plane][y - 1, x] if y > 0 else None)
        return (a + bb + 1) >> 1 if a is not None and bb is not None else a if a is not None else bb if bb is not None else 0
    qp, bits = slice_qp, []
    for m in range(n):
        mx, my = m % mb_w, m // mb_w
        v = b.ue()
        assert 1 <= v <= 24, "macroblock %d: mb_type %d is not an I_16x16 type" % (m, v)
        out["i16mode"][m], chroma, luma15 = (v - 1) % 4, (v - 1) // 4 % 3, (v - 1) // 12
        out["cbp"][m] = (chroma << 4) | (15 if luma15 else 0)
        out["chroma_mode"][m] = b.ue()
        qp = (qp + b.se() + 52) % 52
        out["qp"][m] = qp
        out["luma_dc"][m], _ = residual_block(b, t, n_c(0, 4 * mx, 4 * my), 16)
        for i in range(16 if luma15 else 0):
            x, y = 4 * mx + (i & 1) + 2 * (i >> 2 & 1), 4 * my + (i >> 1 & 1) + 2 * (i >> 3 & 1)
            out["luma"][m, 16 * i + 1:16 * i + 16], tot[0][y, x] = residual_block(b, t, n_c(0, x, y), 15)
        for c in range(2 if chroma else 0):
            out["chroma_dc"][m, 4 * c:4 * c + 4], _ = residual_block(b, t, -1, 4)
        for i in range(8 if chroma == 2 else 0):
            c, x, y = i >> 2, 2 * mx + (i & 1), 2 * my + (i >> 1 & 1)
            out["chroma_ac"][m, 16 * i + 1:16 * i + 16], tot[1 + c][y, x] = residual_block(b, t, n_c(1 + c, x, y), 15)
        bits.append(b.pos)
    assert b.u(1) == 1 and b.pos <= 8 * len(data) and not any(b.u(1) for _ in range(8 * len(data) - b.pos)), "the slice does not end with its trailing bits"
    return out, np.array(bits)
