"""The folder driver (gtcrn_micro_amd/infer.py) on clips that are not at 16 kHz: resampled on the GPU, enhanced, written
at 16 kHz."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import resample_checker as RC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CKPT = os.path.join(GOLDEN, "params_dns3.f32")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as graft
    graft.build()
    return torch.device("cuda:0")


def to_pcm16(x):
    return np.clip(np.rint(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def make_folder(tmp_path, rates, clean_rate=16000):
    """One clip (3 s of reference clip 1) at each rate, made with the float64 checker, written as PCM16."""
    from scipy.io import wavfile
    clip = np.load(os.path.join(GOLDEN, "examples_full.npz"))["noisy"][0, 16000:64000 + 77]
    noisy, clean = tmp_path / "noisy", tmp_path / "clean"
    noisy.mkdir()
    clean.mkdir()
    pcm = {}
    for k, fs in enumerate(rates):
        if fs == 16000:
            x = clip
        else:
            up, down = RC.ratio(16000, fs)
            x = to_pcm16(RC.resample64(clip.astype(np.float64) / 32768.0, up, down, RC.design(16000, fs)[3]))
        pcm[fs] = x
        wavfile.write(str(noisy / f"clip_{fs}_fileid_{k}.wav"), fs, x)
        c = clip if clean_rate == 16000 else np.zeros(RC.out_len(clip.size, *RC.ratio(16000, clean_rate)), np.int16)
        wavfile.write(str(clean / f"clean_fileid_{k}.wav"), clean_rate, c)
    return str(noisy), str(clean), clip, pcm


@pytest.mark.parametrize("pipeline", [True, False])
def test_folder_of_mixed_rates(dev, tmp_path, pipeline):
    """A folder mixing 16, 48, 44.1 and 8 kHz copies of one clip gives 16 kHz files of the clean length.  The 16 kHz one
    is byte-identical to the output of a folder that holds it alone (the existing path); each of the others is
    compared with "that file's PCM16 samples resampled by the float64 checker -> Engine.forward_wave -> the driver's
    PCM16 rounding": within 1 LSB everywhere and equal at >= 99 % of the samples (fp32 resampling error can only move a
    rounding decision).  Measured on MI355X: max 1 LSB; equal at 99.987 % (48 kHz), 99.987 % (44.1 kHz), 99.985 % (8 kHz) of 47 872 samples."""
    from scipy.io import wavfile
    from gtcrn_micro_amd import Engine
    from gtcrn_micro_amd.infer import enhance_folder, load_params
    rates = [16000, 48000, 44100, 8000]
    noisy, clean, clip, pcm = make_folder(tmp_path, rates)
    enh = str(tmp_path / "enh")
    inf_scp, ref_scp = enhance_folder(noisy, clean, enh, CKPT, pipeline=pipeline)
    assert len(inf_scp) == len(rates) == len(ref_scp)
    alone = tmp_path / "alone"
    alone.mkdir()
    n16, c16, _, _ = make_folder(alone, [16000])
    enhance_folder(n16, c16, str(alone / "enh"), CKPT, pipeline=pipeline)
    with open(os.path.join(enh, "clip_16000_fileid_0_enh.wav"), "rb") as a, \
            open(str(alone / "enh" / "clip_16000_fileid_0_enh.wav"), "rb") as b:
        assert a.read() == b.read()
    eng = Engine(load_params(CKPT), 0)
    win = torch.hann_window(512).pow(0.5).cuda()
    for k, fs in enumerate(rates):
        fs_out, y = wavfile.read(os.path.join(enh, f"clip_{fs}_fileid_{k}_enh.wav"))
        assert fs_out == 16000 and y.dtype == np.int16 and y.size == clip.size
        if fs == 16000:
            continue
        up, down = RC.ratio(fs, 16000)
        x16 = RC.resample64(pcm[fs].astype(np.float64) / 32768.0, up, down, RC.design(fs, 16000)[3])
        ref = eng.forward_wave(torch.from_numpy(x16.astype(np.float32)).cuda(), win).cpu().numpy()
        want = to_pcm16(ref)                                    # (x * 32768 is exact: write_wav_pcm16's rounding)
        n = min(want.size, clip.size)
        diff = np.abs(y[:n].astype(np.int32) - want[:n].astype(np.int32))
        share = float((diff == 0).mean())
        print(f"{fs} Hz clip: {n} samples, max |diff| {int(diff.max())} LSB, equal at {100 * share:.3f} %")
        assert not y[n:].any()
        assert diff.max() <= 1
        assert share >= 0.99


def test_reference_file_at_another_rate_counts_with_its_16k_length(dev, tmp_path):
    from scipy.io import wavfile
    from gtcrn_micro_amd.infer import enhance_folder
    noisy, clean, clip, _ = make_folder(tmp_path, [48000], clean_rate=48000)
    enh = str(tmp_path / "enh")
    enhance_folder(noisy, clean, enh, CKPT)
    fs_out, y = wavfile.read(os.path.join(enh, "clip_48000_fileid_0_enh.wav"))
    n48 = RC.out_len(clip.size, 3, 1)
    assert fs_out == 16000 and y.size == RC.out_len(n48, 1, 3) == clip.size


def test_unsupported_rate_still_raises(dev, tmp_path):
    from scipy.io import wavfile
    from gtcrn_micro_amd.infer import enhance_folder
    noisy, clean = tmp_path / "noisy", tmp_path / "clean"
    noisy.mkdir()
    clean.mkdir()
    x = np.zeros(4000, np.int16)
    wavfile.write(str(noisy / "a_fileid_0.wav"), 12345, x)
    wavfile.write(str(clean / "clean_fileid_0.wav"), 16000, x)
    with pytest.raises(AssertionError, match="12345.*48000"):
        enhance_folder(str(noisy), str(clean), str(tmp_path / "enh"), CKPT)
