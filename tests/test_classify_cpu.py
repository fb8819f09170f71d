"""The classifier tail without a device: the parser's two sections and their refusals, the connected packer's layout,
and the weights file that synth writes for them (no kernel is launched)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from yolo_quantization_amd import binding, synth

HEAD = "[net]\nbatch=1\nwidth={w}\nheight={h}\nchannels=3\n\n[convolutional]\nfilters={f}\nsize=1\nstride=1\nactivation=leaky\nquantized=1\n\n"
PARSE = ("import sys; from yolo_quantization_amd import binding; H = binding.host(); "
         "n = H.parse_network_cfg(sys.argv[1].encode(), 0); a = (binding.C.c_int * 16)(); "
         "print([a[0] for i in range(int(sys.argv[2])) if H.dnq_layer_info(n, i, a) == 0])")


def _parse(tmp_path, text, nlayers):
    """parse in a child process (the host's error() ends the process): (exit code, stdout, stderr)"""
    cfg = tmp_path / "t.cfg"
    cfg.write_text(text)
    root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    r = subprocess.run([sys.executable, "-c", PARSE, str(cfg), str(nlayers)], cwd=root, capture_output=True, text=True)
    return r.returncode, r.stdout, r.stderr


def test_parser_accepts_both_sections(tmp_path):
    rc, out, err = _parse(tmp_path, HEAD.format(w=8, h=6, f=24) + "[avg]\nquantized=1\n\n[connected]\noutput=10\nactivation=linear\nquantized=1\n\n"
                          "[conn]\noutput=5\nactivation=relu\nquantized=1\nquant_stop=1\n", 4)
    assert rc == 0 and out.strip() == str([binding.T_CONV, binding.T_AVGPOOL, binding.T_CONNECTED, binding.T_CONNECTED]), err


@pytest.mark.parametrize("w,h,f,tail,msg", [
    (8, 6, 24, "[connected]\noutput=10\nquantized=1\n", "[connected] activation=logistic (or no activation key)"),
    (43, 48, 16, "[connected]\noutput=10\nactivation=leaky\nquantized=1\n", "[connected] K = c h w above 33024"),  # 16 * 43 * 48 = 33024
    (2049, 2048, 16, "[avgpool]\nquantized=1\n", "[avgpool] a map above 2^22 cells")])
def test_parser_refusals(tmp_path, w, h, f, tail, msg):
    if "[connected] K" in msg:  # K = 33024 parses, one channel more is refused
        assert _parse(tmp_path, HEAD.format(w=w, h=h, f=f) + tail, 2)[0] == 0
        f += 1
    rc, out, err = _parse(tmp_path, HEAD.format(w=w, h=h, f=f) + tail, 2)
    assert rc != 0 and msg in err


@pytest.mark.parametrize("Cc,H,W,n", [(24, 2, 3, 17), (16, 7, 7, 5), (80, 1, 1, 33)])
def test_connected_pack_round_trips(Cc, H, W, n):
    """[M tile][K step][lane = q * 16 + m][16 B]: byte e is packed K 64 step + 16 q + e of filter 16 tile + m; packed K = cell * cs + channel
    with cs the 16-byte pieces of a cell that hold channels, whatever cell size the blob is packed for"""
    rng = np.random.default_rng(n)
    cs, hw = (Cc + 15) // 16 * 16, H * W
    wq = rng.integers(0, 256, (n, Cc * hw), dtype=np.uint8)
    args = (rng.integers(0, 256, n, dtype=np.uint8), Cc, H, W)
    blob = binding.connected_pack(wq, *args, cs, np.zeros(n, np.int32), np.full(n, 0.5), np.full(n, 2.0 ** -9))
    assert blob.size == binding.shim().mi355_connected_pack_size(n, Cc, H, W, cs)
    assert np.array_equal(blob, binding.connected_pack(wq, *args, cs + 32, np.zeros(n, np.int32), np.full(n, 0.5), np.full(n, 2.0 ** -9)))
    mtiles, nsteps = (n + 15) // 16, (hw * cs + 63) // 64
    frag = blob[64:64 + mtiles * nsteps * 1024].view(np.int8).reshape(mtiles, nsteps, 4, 16, 16)  # tile, step, q, m, byte
    got = frag.transpose(0, 3, 1, 2, 4).reshape(mtiles * 16, nsteps * 64)                         # [filter][packed K]
    want = np.zeros_like(got)
    cells = np.zeros((n, hw, cs), np.int8)
    cells[:, :, :Cc] = (wq.reshape(n, Cc, hw).transpose(0, 2, 1) ^ 0x80).view(np.int8)            # (c, y, x) -> (y, x, channel), w - 128
    want[:n, :hw * cs] = cells.reshape(n, -1)
    assert np.array_equal(got, want)


def test_synth_and_load_weights_agree_on_the_file(cfg_dir, tmp_path, capfd):
    cfg, wts = os.path.join(cfg_dir, "cls_unit.cfg"), str(tmp_path / "cls_unit.weights")
    made = synth.synth_weights(cfg, wts, seed=1)
    assert [r["K"] for r in made["layers"]][-2:] == [40, 24] and os.path.getsize(wts) == made["bytes"]
    H = binding.host()
    net = H.load_network(cfg.encode(), wts.encode(), 0)
    assert net and "trailing bytes" not in capfd.readouterr().err
