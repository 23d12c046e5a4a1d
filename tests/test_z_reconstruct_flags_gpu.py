"""GPU: the command-line entry of the spectral track join -- reconstruct.py --join spectral --stretch R on a generated wav with a
seeded small checkpoint, in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from phasegen import detgen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_join_spectral_with_stretch(tmp_path):
    from scipy.io import wavfile
    from phasegen.model import UNetModel
    weight, wav_in, wav_out = tmp_path / "unet.pth", tmp_path / "in.wav", tmp_path / "out.wav"
    UNetModel(16, 32, gpu_ids=[0]).load_numpy(detgen.make_params(16, seed=0)).save(str(weight))
    wavfile.write(wav_in, 16000, np.round(detgen.make_clip(1000, seed=61) * 20000).astype(np.int16))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "unet-phasegen_amd", "reconstruct.py"), "--weight", str(weight),
                        "--input", str(wav_in), "--output", str(wav_out), "--channels", "16", "--frames", "24", "--overlap_frames", "4",
                        "--join", "spectral", "--stretch", "1.25"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Reconstructed ")]
    assert len(lines) == 1 and lines[0].endswith(" s (9 clips).")                   # 1250 samples: 1 + ceil(1066 / 152)
    sr, out = wavfile.read(wav_out)
    assert sr == 16000 and out.dtype == np.float32 and out.shape == (1250,)
    assert np.isfinite(out).all() and float(np.abs(out).max()) == 1.0
