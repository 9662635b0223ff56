"""Pure-numpy mirror of the queue tracks (csrc/des_tracks.hip, simlog_to_vid.log_tracks) and of simlog_to_vid.bar_frames:
the rule written down a second time, record by record and pixel by pixel, with none of the package's code."""
import numpy as np

ARRIVAL, DEPARTURE = 0, 1
ENODE, EPTR = 1, 2
VIRIDIS = [(68, 1, 84), (71, 44, 122), (59, 81, 139), (44, 113, 142), (33, 144, 141), (39, 173, 129), (92, 200, 99),
           (170, 220, 50), (253, 231, 37)]


def tracks_of(node, kind, servers, max_lines=5000):
    """One log -> (rows (n, S) int32, status).  A status gives zero rows."""
    counters = {int(s): 0 for s in servers}
    rows = [[0] * len(servers)]
    for line, (nd, kd) in enumerate(zip(np.asarray(node).tolist(), np.asarray(kind).tolist())):
        if line >= max_lines:
            break
        if kd not in (ARRIVAL, DEPARTURE):
            continue
        if nd not in counters:
            return np.zeros((0, len(servers)), dtype=np.int32), ENODE
        counters[nd] += 1 if kd == ARRIVAL else -1
        if sum(counters.values()) > 0:
            rows.append([counters[int(s)] for s in servers])
    return np.array(rows, dtype=np.int32).reshape(-1, len(servers)), 0


def batch_tracks(node, kind, rec_ptr, servers, max_lines=5000):
    """B logs in CSR form, servers (B, S) -> (tracks, row_ptr, status)."""
    parts, status, row_ptr = [], [], [0]
    for b in range(len(rec_ptr) - 1):
        lo, hi = int(rec_ptr[b]), int(rec_ptr[b + 1])
        rows, st = tracks_of(node[lo:hi], kind[lo:hi], servers[b], max_lines)
        parts.append(rows)
        status.append(st)
        row_ptr.append(row_ptr[-1] + len(rows))
    return np.concatenate(parts), np.array(row_ptr, dtype=np.int64), np.array(status, dtype=np.int32)


def bar_frames(tracks, height=480, width=640):
    tracks = np.asarray(tracks)
    t_n, s = tracks.shape
    top, left = height // 10, width // 10
    ph, pw = height - 2 * top, width - 2 * left
    palette = [(255, 255, 255), (0, 0, 0)]
    for j in range(s):
        x = (j / (s - 1) if s > 1 else 0.0) * 8
        lo = min(int(x), 7)
        f = x - lo
        palette.append(tuple(int(np.floor(VIRIDIS[lo][c] * (1.0 - f) + VIRIDIS[lo + 1][c] * f + 0.5)) for c in range(3)))
    frames = np.zeros((t_n, height, width), dtype=np.uint8)
    ylim = 0.0
    for t in range(t_n):
        img = frames[t]
        for x in range(left - 1, left + pw + 1):
            img[top - 1, x] = img[top + ph, x] = 1
        for y in range(top - 1, top + ph + 1):
            img[y, left - 1] = img[y, left + pw] = 1
        ylim = max(1.1 * float(max(tracks[t])), ylim)
        for j in range(s):
            v = float(tracks[t, j])
            if v <= 0 or ylim <= 0:
                continue
            h = min(int(ph * v / ylim), ph)
            for y in range(top + ph - h, top + ph):
                img[y, left + (10 * j + 1) * pw // (10 * s):left + (10 * j + 9) * pw // (10 * s)] = 2 + j
    return frames, np.array(palette, dtype=np.uint8)
