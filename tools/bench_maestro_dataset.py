"""Timing of model 1's MAESTRO route.  On an MI355X:

    python tools/bench_maestro_dataset.py [OUT.json]

A generated MAESTRO-shaped folder with one ten-minute, 20 000-note performance (two tracks, tempo changes, sustain pedal
every few notes; about 120 five-second windows, of which an item keeps 30).  One warm-up, then three timed repetitions of
  item   datasets.MaestroDataset(30, ...)[0]: file on disk -> (30, 128, 216) mel-dB tensor on the device
  host   its host part alone: datasets.read_midi + datasets.midi_notes on the same file
alternated, each ending in a device synchronise; medians.  Figures are printed as JSON (and written to OUT.json),
nothing is asserted."""
import json, os, random, statistics, struct, sys, tempfile, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_des_midi_music_gen_amd import datasets


def vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes(reversed(out))


def track(events):                                     # [(absolute tick, bytes)] -> an MTrk chunk
    body, now = bytearray(), 0
    for tick, data in sorted(events, key=lambda e: e[0]):
        body += vlq(tick - now) + data
        now = tick
    body += b"\x00\xff\x2f\x00"
    return b"MTrk" + struct.pack(">I", len(body)) + bytes(body)


g = np.random.default_rng(0)
n_notes, seconds, tpb = 20000, 600, 480                # default tempo: 960 ticks per second
ons = np.sort(g.integers(0, seconds * 960 - 2000, n_notes))
events = []
for k, on in enumerate(ons.tolist()):
    pitch, vel = int(g.integers(21, 109)), int(g.integers(20, 120))
    events.append((on, bytes([0x90, pitch, vel])))
    events.append((on + int(g.integers(40, 1500)), bytes([0x80, pitch, 64])))
    if k % 5 == 0:
        events.append((on, bytes([0xB0, 64, 127 if (k // 5) % 2 == 0 else 0])))
tempi = [(t, b"\xff\x51\x03" + int(500000 + 20 * (t % 977)).to_bytes(3, "big")) for t in range(0, seconds * 960, 9600)]
root = tempfile.mkdtemp()
with open(os.path.join(root, "performance.midi"), "wb") as f:
    f.write(b"MThd" + struct.pack(">IHHH", 6, 1, 2, tpb) + track(tempi) + track(events))
with open(os.path.join(root, "maestro-v3.0.0.json"), "w") as f:
    json.dump({"midi_filename": {"0": "performance.midi"}}, f)
path = os.path.join(root, "performance.midi")
ds = datasets.MaestroDataset(30, input_folder=root)


def item():
    random.seed(0)
    spec = ds[0]
    torch.cuda.synchronize()
    return spec


def host():
    return datasets.midi_notes(datasets.read_midi(path))


spec = item()                                          # warm-up (code objects, constant matrices)
notes, clip_len = host()
times = {"item": [], "host": [], "read_midi": []}
for rep in range(3):
    for name, fn in (("item", item), ("host", host), ("read_midi", lambda: datasets.read_midi(path))):
        t0 = time.perf_counter(); fn(); times[name].append((time.perf_counter() - t0) * 1e3)
res = {"file": {"bytes": os.path.getsize(path), "notes": len(notes), "clip_seconds": clip_len / 44100,
                "item_shape": list(spec.shape)},
       "item_ms": times["item"], "host_ms": times["host"], "read_midi_ms": times["read_midi"],
       "item_median_ms": statistics.median(times["item"]), "host_median_ms": statistics.median(times["host"]),
       "read_midi_median_ms": statistics.median(times["read_midi"])}
print(json.dumps(res))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
