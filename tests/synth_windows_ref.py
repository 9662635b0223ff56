"""numpy restatement of gdm_synth_windows, written from the text of include/gdm.h -- TEST INFRASTRUCTURE ONLY.

Rows are (s_on, s_off, pitch, velocity) with the times in samples.  A voice contributes at s in [s_on, s_off + R):
    phase = uint32(inc[p] * (s - s_on));  e_att = min(s - s_on + 1, A);  e_rel = R if s < s_off else R - (s - s_off)
    voice = (wave[phase >> 21] * v * e_att * e_rel) >> SHIFT          (arithmetic shift)
and a sample is the sum of its voices clamped to the 16-bit range.  int64 arithmetic, a plain loop over the voices, the
clamp at the end; nothing of the kernel's searches, tiles or rebasing is restated.
"""
import struct

import numpy as np

ATTACK, RELEASE, SHIFT, WAVE_LEN, RATE = 256, 8192, 30, 2048, 44100


def tables():
    """(wave int16[2048], inc uint32[128]) as the host builds them, in float64."""
    i = np.arange(WAVE_LEN, dtype=np.float64)
    wave = np.round(32767.0 * np.sin(2.0 * np.pi * i / WAVE_LEN)).astype(np.int16)
    p = np.arange(128, dtype=np.float64)
    inc = np.round(2.0 ** 32 * 440.0 * 2.0 ** ((p - 69.0) / 12.0) / RATE).astype(np.uint32)
    return wave, inc


_TABLES = tables()


def voice_sum(notes, start, count):
    """int64 (count,): the unclamped sum of the voices at samples start .. start + count."""
    wave, inc = _TABLES
    wave = wave.astype(np.int64)
    s = np.arange(start, start + count, dtype=np.int64)
    total = np.zeros(count, dtype=np.int64)
    for s_on, s_off, pitch, vel in np.asarray(notes, dtype=np.int64).reshape(-1, 4).tolist():
        a, b = max(s_on, start), min(s_off + RELEASE, start + count)
        if a >= b:
            continue
        t = s[a - start:b - start]
        d = t - s_on
        phase = (d * int(inc[pitch & 127])) & 0xFFFFFFFF            # an int64 product that wraps keeps its low 32 bits
        e_att = np.minimum(d + 1, ATTACK)
        e_rel = np.where(t < s_off, RELEASE, RELEASE - (t - s_off))
        total[a - start:b - start] += (wave[phase >> 21] * (vel & 127) * e_att * e_rel) >> SHIFT
    return total


def window(notes, start, count):
    """int16 (count,): samples start .. start + count of the clip."""
    total = voice_sum(notes, start, count)
    assert np.abs(total).max(initial=0) < 1 << 31, "the kernel's int32 sum would overflow"
    return np.clip(total, -32768, 32767).astype(np.int16)


def windows(clips, win_clip, win_start, win_len):
    """(W, win_len) int16: window w = samples win_start[w] .. + win_len of clips[win_clip[w]]."""
    return np.stack([window(clips[c], s, win_len) for c, s in zip(win_clip, win_start)])


def off_max(notes):
    """The running maximum of s_off over one clip's rows."""
    return np.maximum.accumulate(np.asarray(notes, dtype=np.int64).reshape(-1, 4)[:, 1])


def as_gm(notes, seed):
    """The clip as gdm_synth_windows_gm takes it when every family has the plain voice (``plain_gm_tables``): a fifth
    column of seeded programs 0..127, and end_max = off_max + RELEASE."""
    notes = np.asarray(notes, dtype=np.int64).reshape(-1, 4)
    programs = np.random.default_rng(seed).integers(0, 128, (len(notes), 1))
    return np.concatenate([notes, programs], axis=1), off_max(notes) + RELEASE


def plain_gm_tables():
    """(waves (16, 2048), env (16, 2), inc) of gdm_synth_windows_gm under which it is gdm_synth_windows: the one wave
    table and (ATTACK, RELEASE) for every family."""
    wave, inc = _TABLES
    return np.tile(wave, (16, 1)), np.tile(np.asarray([ATTACK, RELEASE], dtype=np.int64), (16, 1)), inc


# ---- hand-assembled Standard MIDI Files ----------------------------------------------------------------------------------
def _vlq(n):
    assert 0 <= n < 1 << 28
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes(reversed(out))


_STATUS = {"off": 0x80, "on": 0x90, "cc": 0xB0, "pc": 0xC0}


def midi_bytes(tracks, ticks_per_beat=480):
    """A format-1 file of ``tracks``, each a list of (delta ticks, message): ("on" | "off" | "cc", channel, a, b),
    ("pc", channel, program), ("tempo", us per beat).  Channel messages use running status; every track gets its
    end_of_track, ``("eot",)`` places it explicitly (with its delta)."""
    chunks = []
    for track in tracks:
        body, running = bytearray(), None
        ended = False
        for delta, msg in track:
            body += _vlq(delta)
            if msg[0] == "tempo":
                body += b"\xff\x51\x03" + int(msg[1]).to_bytes(3, "big")
                running = None
            elif msg[0] == "eot":
                body += b"\xff\x2f\x00"
                ended = True
            else:
                status = _STATUS[msg[0]] | msg[1]
                if status != running:
                    body.append(status)
                body += bytes(msg[2:])
                running = status
        if not ended:
            body += b"\x00\xff\x2f\x00"
        chunks.append(b"MTrk" + struct.pack(">I", len(body)) + bytes(body))
    return b"MThd" + struct.pack(">IHHH", 6, 1, len(tracks), ticks_per_beat) + b"".join(chunks)
