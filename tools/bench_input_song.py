"""Timing of model 1's file input.  On an MI355X:

    python tools/bench_input_song.py [OUT.json]

A generated 60-second stereo 16-bit file at 44.1 kHz (13 windows of 5 s), two routes from the file on disk to the
(N, 128, 216) mel-dB tensor on the device, alternated, one warm-up and three timed repetitions each, medians:
  input_song  datasets.InputSong(file).spectrograms(): load_wav, one upload of the sample bytes, gdm_pcm_stft_frames
  host        what a user does without it: wave + numpy decode of channel 0 and slicing into windows, upload of the
              stacked float windows, util.get_melspectrogram_db_tensor
Both end in a device synchronise.  Figures are printed as JSON (and written to OUT.json), nothing is asserted except that
the two routes return the same bits."""
import json, os, statistics, sys, tempfile, time, wave
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_des_midi_music_gen_amd import datasets, util

rate, seconds = 44100, 60
n = rate * seconds
g = np.random.default_rng(0)
t = np.arange(n) / rate
song = np.stack([0.4 * np.sin(2 * np.pi * 440.0 * t * (1 + 0.01 * t)), 0.3 * np.sin(2 * np.pi * 1250.0 * t)], axis=1)
song = np.round((song + 0.02 * g.standard_normal((n, 2))) * 32767.0).clip(-32768, 32767).astype("<i2")
path = os.path.join(tempfile.mkdtemp(), "song.wav")
with wave.open(path, "wb") as w:
    w.setnchannels(2); w.setsampwidth(2); w.setframerate(rate); w.writeframes(song.tobytes())


def input_song():
    spec = datasets.InputSong(path).spectrograms()
    torch.cuda.synchronize()
    return spec


def host():
    with wave.open(path) as w:
        sr = w.getframerate()
        raw = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, w.getnchannels())
    left = raw[:, 0].astype(np.float32) / 32768.0
    cut = [left[s:s + m] for s, m in util.song_windows(len(left), sr)]
    spec = util.get_melspectrogram_db_tensor(torch.from_numpy(np.stack(cut)).cuda(), sr=sr)
    torch.cuda.synchronize()
    return spec


a, b = input_song(), host()                      # warm-up of both routes (code objects, constant matrices)
assert torch.equal(a.view(torch.int32), b.view(torch.int32))
times = {"input_song": [], "host": []}
for rep in range(3):                             # alternate the routes
    for name, fn in (("input_song", input_song), ("host", host)):
        t0 = time.perf_counter(); fn(); times[name].append((time.perf_counter() - t0) * 1e3)
res = {"file": {"seconds": seconds, "rate": rate, "channels": 2, "bytes": os.path.getsize(path), "windows": len(a)},
       "input_song_ms": times["input_song"], "host_ms": times["host"],
       "input_song_median_ms": statistics.median(times["input_song"]), "host_median_ms": statistics.median(times["host"])}
print(json.dumps(res))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
