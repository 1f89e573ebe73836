"""Float64 NumPy restatement of sedt_cut_clips (include/sedt_hip.h; DESIGN.md section 4, "Training on recordings"), written from the
definition, not from the kernel: no binary search, no chunks - every event of the recording is looked at, in table order.

Wave: row b = samples start[b] .. start[b] + window - 1 of recording rec[b]; positions past the recording's end are zero.
Targets: W = window / sr, t0 = start[b] / sr, t1 = t0 + W; for every event (c, on, end) of the recording in table order
a = max(on, t0) - t0, z = min(end, t1) - t0; kept iff z - a > 0 and z - a >= min_event_seconds; label c (int64), box
(float32(((a + z) * 0.5) / W), float32((z - a) / W)).  More than max_targets survivors: status 1, the first max_targets are written.
Blob: int32 lab_off [B + 1] | box_off [B + 1] | B | B, lab_cat int64 at byte 8 B + 16, box_cat float32 pairs behind its B * max_targets
entries; box_off == lab_off, exclusive scans over the clips."""
import numpy as np


def clip_targets(table, r, start, window, sr, max_targets, min_event_seconds=0.0):
    """(labels int64 (n,), boxes float32 (n, 2), status) of one clip; ``table``: what utilities.recording_clips.clip_event_table
    returns ('off' per recording, 'on', 'end', 'cls')"""
    W = np.float64(window) / np.float64(sr)
    t0 = np.float64(start) / np.float64(sr)
    t1 = t0 + W
    labels, boxes, status = [], [], 0
    for j in range(int(table['off'][r]), int(table['off'][r + 1])):
        on, end = np.float64(table['on'][j]), np.float64(table['end'][j])
        a = max(on, t0) - t0
        z = min(end, t1) - t0
        d = z - a
        if not (d > 0 and d >= np.float64(min_event_seconds)):
            continue
        if len(labels) == max_targets:
            status = 1
            break
        labels.append(int(table['cls'][j]))
        boxes.append((np.float32(((a + z) * np.float64(0.5)) / W), np.float32(d / W)))
    return np.asarray(labels, np.int64), np.asarray(boxes, np.float32).reshape(-1, 2), status


def cut_clips(recordings, table, rec, start, window, sr, max_targets, min_event_seconds=0.0):
    """recordings: list of 1-D float32 arrays.  Returns (wave float32 [B, window], [(labels, boxes)] per clip, status int32 [B])"""
    B = len(rec)
    wave = np.zeros((B, window), np.float32)
    targets, status = [], np.zeros(B, np.int32)
    for b in range(B):
        src = recordings[int(rec[b])][int(start[b]):int(start[b]) + window]
        wave[b, :len(src)] = src
        lab, box, status[b] = clip_targets(table, int(rec[b]), int(start[b]), window, sr, max_targets, min_event_seconds)
        targets.append((lab, box))
    return wave, targets, status


def blob(targets, max_targets):
    """the target blob as (off int32 [2 B + 4], lab_cat int64 [n], box_cat float32 [n, 2], byte offsets (o_lab, o_box, total))"""
    B = len(targets)
    counts = [len(t[0]) for t in targets]
    lab_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    off = np.concatenate([lab_off, lab_off, [B, B]]).astype(np.int32)
    lab = np.concatenate([t[0] for t in targets]) if B else np.zeros(0, np.int64)
    box = np.concatenate([t[1] for t in targets]) if B else np.zeros((0, 2), np.float32)
    o_lab = 8 * B + 16
    o_box = o_lab + 8 * B * max_targets
    return off, lab.astype(np.int64), box.astype(np.float32).reshape(-1, 2), (o_lab, o_box, o_box + 8 * B * max_targets)
