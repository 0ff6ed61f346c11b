"""GPU tests of the wide walk inside the resident routes (run with -m gpu on an MI355X): Decoder.decode_resident_tensor,
decode_wav_resident and block_index_resident with the handle option "wide_walk" on, against the same calls with it off
-- the lane walk, which is the code path the option replaces.  Tensors, sample counts, codes and WAV bytes must be equal;
Decoder.last_walk() must show the route taken."""
import numpy as np
import pytest

import slalibs as S
import test_gpu_decode_batch as TB
import test_gpu_decode_batch_resident as TR
import walkmodel as WM

pytestmark = pytest.mark.gpu

LONG = S.make_params(1, 16, 48000, 16, 1, 8, 0, 1, 2048, cap=(2, 4096, 16, 1, 8))      # mono, 2048-sample blocks


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


@pytest.fixture(scope="module")
def files(hip):
    """a file of a few hundred blocks and five short stereo clips"""
    long = TB.encode_clips(hip, LONG, [S.synth_pcm(1, 600000, 16, 48000, seed=41)])[0]
    lens = [6000, 9001, 12345, 20000, 5000]
    clips = TB.encode_clips(hip, TB.C4, [S.synth_pcm(2, n, 16, 48000, seed=950 + i) for i, n in enumerate(lens)])
    blocks = WM.walk(long, 600000, 600000, 8192).num_blocks
    assert 250 <= blocks <= 1000
    return long, clips, blocks


def _both(dec, call, routes):
    """call() with "wide_walk" 0 and then with each (wide_walk, wide_walk_nodes) of routes; -> the results, last_walk()s"""
    out, walks = [], []
    for wide, nodes in [(0, 0)] + list(routes):
        dec.set_option("wide_walk", wide)
        dec.set_option("wide_walk_nodes", nodes)
        out.append(call())
        walks.append(dec.last_walk())
    dec.set_option("wide_walk", 0)
    dec.set_option("wide_walk_nodes", 0)
    assert walks[0] == (0, 0, 0, 0)
    return out, walks


def _same_tensors(a, b):
    import torch
    return torch.equal(a[0], b[0]) and a[1:] == b[1:]


@pytest.mark.parametrize("batch", [False, True])
def test_tensors_of_a_long_file_alone_and_among_short_clips(hip, files, batch):
    import torch
    long, clips, blocks = files
    datas = clips[:3] + [long] + clips[3:] if batch else [long]
    srcs, keep = TR.resident(datas)
    dec = TB.make_decoder(hip)
    try:
        routes = [(1, 0), (len(long), 0), (1, 1), (len(long), blocks)]
        out, walks = _both(dec, lambda: dec.decode_resident_tensor(srcs, dtype=torch.int32), routes)
        assert all(rc == 0 for rc in out[0][2]) and 600000 in out[0][1]
        for o in out[1:]:
            assert _same_tensors(o, out[0])
        n = len(datas)
        assert walks[1][:2] == (n, 0) and walks[1][2] >= blocks and walks[1][3] > 0          # every file wide
        assert walks[2][:2] == (1, 0) and walks[2][2] >= blocks                              # only the long one
        assert walks[3][:2] == (n, n) and walks[3][2] == walks[1][2]                         # capacity 1: all fall back
        assert walks[4][0] == 1 and walks[4][1] in (0, 1)                                    # capacity = its blocks
        assert walks[4][1] == (1 if walks[2][2] > blocks else 0)                             # overflow iff it has decoys
    finally:
        dec.close()


def test_wav_files_of_a_long_file_among_short_clips(hip, files):
    long, clips, blocks = files
    datas = [clips[0], long, clips[1]]
    srcs, keep = TR.resident(datas)
    dec = TB.make_decoder(hip)
    try:
        call = lambda: [(rc, bytes(t.cpu().numpy())) for rc, t in dec.decode_wav_resident(srcs)]
        out, walks = _both(dec, call, [(len(long), 0), (1, 1)])
        assert [rc for rc, _ in out[0]] == [0, 0, 0] and len(out[0][1][1]) == 44 + 2 * 600000
        assert out[1] == out[0] and out[2] == out[0]
        assert walks[1][:2] == (1, 0) and walks[2][:2] == (3, 3)
    finally:
        dec.close()


def test_a_file_damaged_mid_chain(hip, files):
    import torch
    long, clips, blocks = files
    rows = WM.walk(long, 600000, 600000, 8192).rows
    mid = rows[blocks // 2][0]
    lost = bytearray(long); lost[mid] = 0x7F                                   # no sync code at a block mid-chain
    far = bytearray(long); far[mid + 2:mid + 6] = (len(long)).to_bytes(4, "big")  # a size field beyond the end
    short = long[:rows[blocks - 3][0] + 5]                                     # the stream ends inside a header
    datas = [bytes(lost), clips[0], bytes(far), short]
    srcs, keep = TR.resident(datas)
    dec = TB.make_decoder(hip)
    try:
        out, walks = _both(dec, lambda: dec.decode_resident_tensor(srcs, dtype=torch.int32), [(len(short), 0)])
        assert _same_tensors(out[1], out[0])
        assert out[0][2][0] != 0 and out[0][2][2] != 0 and out[0][2][3] != 0 and out[0][2][1] == 0
        assert out[0][1][0] == rows[blocks // 2][2] and out[0][1][3] == rows[blocks - 3][2]   # the samples in front of the damage
        assert walks[1][:2] == (3, 0)
    finally:
        dec.close()


def test_ten_long_files_eight_go_wide(hip, files):
    import torch
    long, clips, blocks = files
    rows = WM.walk(long, 600000, 600000, 8192).rows
    datas = [long[:rows[40 + k][0]] for k in range(10)]                        # ten lengths, 40 to 49 blocks
    srcs, keep = TR.resident(datas)
    dec = TB.make_decoder(hip)
    try:
        out, walks = _both(dec, lambda: dec.decode_resident_tensor(srcs, dtype=torch.int32), [(1000, 0)])
        assert _same_tensors(out[1], out[0])
        assert out[0][1] == [rows[40 + k][2] for k in range(10)]
        assert walks[1][:2] == (8, 0)
    finally:
        dec.close()


def test_block_index_wide_equals_lane(hip, files):
    long, clips, blocks = files
    srcs, keep = TR.resident([clips[0], long, clips[1]])
    dec = TB.make_decoder(hip)
    try:
        lane = dec.block_index_resident(srcs, wide=False)
        assert len(lane[1][0]) == blocks and lane[1][2] == 0

        def same(got):
            return all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] for a, b in zip(got, lane))
        assert same(dec.block_index_resident(srcs, wide=True))
        assert dec.last_walk()[:2] == (3, 0) and dec.last_walk()[2] >= blocks
        assert same(dec.block_index_resident(srcs))                            # the handle's threshold: off
        assert dec.last_walk() == (0, 0, 0, 0)
        dec.set_option("wide_walk", len(long))
        assert same(dec.block_index_resident(srcs))
        assert dec.last_walk()[:2] == (1, 0)
        dec.set_option("wide_walk_nodes", 1)
        assert same(dec.block_index_resident(srcs, wide=True))                 # every walk overflows and falls back
        assert dec.last_walk()[:2] == (3, 3)
    finally:
        dec.close()
