"""Training soundscapes synthesized on the device.  Both corpora of the reference (URBAN-SED, DESED's synthetic subset) were made by
laying isolated foreground sounds over background recordings at drawn onsets and signal-to-noise ratios; the generator wrote the
annotations and data_utils/collapse_event.py merged them per class.  Here a bank of such sounds is staged on the device ONCE and every
training batch is a fresh set of soundscapes: the host draws a plan (which sounds, where, how loud), ONE call mixes the B clips and
builds their target tables (sedt_soundscape, csrc/soundscape.hip) in the layout sedt_cut_clips writes, so DeviceTargets, TargetTables.load
and load_mixed take them unchanged.  DESIGN.md section 4 ("Soundscapes synthesized on the device") holds the definition;
tests/soundscape_ref.py restates it.

    scapes = SoundscapeClips(mel, labels, window_seconds=10.0)
    scapes.add_events(sounds, ['Speech', 'Dog', ...]).add_backgrounds(rooms)
    x, targets = scapes.batch(transform, scapes.draw(64))        # (B, 1, frames, n_mels), DeviceTargets - nothing synchronises
    engine.train_on_recordings(step, scapes, transform, steps)    # the plain loop takes it as it takes a RecordingClips

The plan.  ``draw`` consumes np.random clip by clip, in this order (a seed fixes the plan):
    background  bi = randint(n_backgrounds), start = randint(len_bg)                   (nothing is drawn with background=False)
    K = randint(lo, hi + 1) events; for each:  c = randint(number of classes that have sounds) - the c-th such class, ascending;
        s = randint(sounds of that class); snr = uniform(snr_lo, snr_hi); n = min(len_src, max_event_samples, window);
        src_start = randint(len_src - n + 1); onset = randint(window - n + 1)
    With ``pitch_shift=(lo, hi)`` and / or ``time_stretch=(lo, hi)`` (the generator's two event effects; utilities/stretch.py), right
    after snr and in the generator's order:  p = uniform(pitch range) semitones if pitch_shift is given, then f = uniform(stretch range)
    if time_stretch is given - both stored as float32 in the plan's ``fx``; n = the largest excerpt whose final length
    m = floor(n f + 0.5) fits min(len_src f, max_event_samples, window); src_start as above; onset = randint(window - m + 1).  With both
    None nothing new is drawn: the plan of a seed is the plan it always was.  ``mix`` runs the effects on the device (sedt_stretch)
    into a buffer behind the bank and hands the unchanged mixing call one more source per transformed event; without ``relevel`` an
    event's gain stays what its SOURCE's staged level gives.
Gains are computed in float64 and stored as float32: g_bg = 10^(ref_db / 20) / rms_bg (1 for a silent background),
g_ev = 10^((ref_db + snr) / 20) / rms_src, the RMS taken over the WHOLE source - the default, ``level='rms'``.  With ``level='lufs'``
the reference is the source's BS.1770 loudness L as Scaper's is (utilities/loudness.py, measured on the device when the source is
staged): 10^(L / 20) stands where the RMS stands, so g = 10^((ref_db + snr - L) / 20), and ref_db and snr are LUFS values.  Nothing
else changes: the same draws in the same order, the same mixing.  fade = round(fade_seconds * sr) samples of linear ramp at both ends
of an event.
    With ``reverb=True`` or ``reverb=prob`` (0 < prob <= 1) and room impulse responses staged (``add_rirs``; utilities/reverb.py) the plan
    gains ``rir``, int32 [E], -1: dry.  Per clip, right after the background draw: room = randint(n_rooms).  Per event, right after the
    effect draws and before src_start: with a probability, uniform() < prob decides whether the event is wet (``True`` draws nothing
    here); a wet event then draws rir = the room's responses[randint(count)], a dry one draws nothing more.  n, m and the onset are
    drawn as before: the tail is NOT made to fit the window.  With reverb=None nothing new is drawn.  ``mix`` runs sedt_reverb behind
    the stretch stage, over the wet events: a wet event's first m samples (the head) go to the mixing call as the event - same onset,
    class and gain, fade 0, the stage applied the fades to the dry sound - so the annotations stay those of the dry event; its last
    L - 1 samples (the tail) are laid, with the event's gain, over the clip's background in a bed row of ``window`` samples
    (sedt_reverb_bed) that becomes the clip's background record (row, 0, 1.0).  Backgrounds stay dry, and the tail past the window's
    end is cut.
    With ``relevel=True`` (the constructor's default, or ``mix(plan, relevel=)``) the level of every event is measured AFTER its effects,
    as the generators do (utilities/relevel.py, sedt_relevel: ONE launch behind the stretch and reverb stages, nothing read back): the
    region is the whole wet row of a wet event (n + L - 1 samples; the fades are in it), the row of m samples of a stretched one, the
    bank excerpt [src_start, src_start + n) of any other - the fades of dry and stretched events are not part of the measurement.  The
    gain float32(target / sqrt(level)) replaces the host's in the DEVICE records of the event and of its tail, target_db = ref_db + snr
    per event (the plan's ``target_db``; draw_plan always fills it and consumes no randomness for it).  A region that is silent or
    under the absolute gate keeps the host's gain (``last_relevel``: the stage's level, counts and status on the device).  Backgrounds
    loop from a random start, so their whole-source level stays the right one; the peak limit and the targets are untouched.

``draw_plan``, ``make_plan``, ``gains`` and the record dtypes are the host half and need no GPU."""
import math

import numpy as np
import torch

from .. import lib as L
from .recording import stage_recordings, stage_resampled
from .recording_clips import DeviceTargets, blob_layout
from .transforms import PinnedRing

# the device records of sedt_soundscape (include/sedt_hip.h: SedtScapeEvent 40 bytes, SedtScapeBg 24 bytes; sedt_sizeof 13 and 14)
EVENT = np.dtype([('src', '<i4'), ('cls', '<i4'), ('src_start', '<i8'), ('n', '<i8'), ('onset', '<i8'), ('gain', '<f4'), ('fade', '<i4')])
BACKGROUND = np.dtype([('src', '<i4'), ('pad', '<i4'), ('start', '<i8'), ('gain', '<f4'), ('pad2', '<i4')])
# an event's effects (host only: the device sees SedtStretchJob records, utilities/stretch.py); (0, 1) is the identity
FX = np.dtype([('semitones', '<f4'), ('factor', '<f4')])
STATUS_REASONS = {1: 'more events survive in the clip than max_targets holds: build SoundscapeClips with a larger max_targets',
                  2: 'a record of the clip does not lie inside the bank (or the clip holds more than 63 events)'}


class SoundscapePlan(object):
    """the records of B soundscapes as sedt_soundscape reads them: ``bg`` BACKGROUND [B] (src -1: no background), ``ev`` EVENT [E],
    ``ev_off`` int32 [B + 1] - clip b's events are ev[ev_off[b]:ev_off[b + 1]], mixed in that order.  ``fx``: None (no effects) or FX [E],
    the pitch shift and duration factor of every event; an event's ``n`` is then the length of its EXCERPT, and it occupies
    floor(n factor + 0.5) samples of the clip from ``onset`` on.  ``rir``: None (all dry) or int32 [E], the room impulse response every
    event is convolved with, -1: dry.  ``target_db``: None or float64 [E], the level every event shall have in the clip - ref_db + snr, in
    dB of its RMS or in LUFS as the bank's ``level`` says; read only when the plan is mixed with ``relevel``"""

    def __init__(self, bg, ev, ev_off, fx=None, rir=None, target_db=None):
        self.bg = np.ascontiguousarray(bg, BACKGROUND)
        self.ev = np.ascontiguousarray(ev, EVENT)
        self.ev_off = np.ascontiguousarray(ev_off, np.int32)
        self.fx = None if fx is None else np.ascontiguousarray(fx, FX)
        self.rir = None if rir is None else np.ascontiguousarray(rir, np.int32)
        self.target_db = None if target_db is None else np.ascontiguousarray(target_db, np.float64)
        B = self.bg.shape[0]
        if self.bg.shape != (B,) or self.ev_off.shape != (B + 1,) or self.ev.ndim != 1:
            raise ValueError('SoundscapePlan: bg [B], ev [E], ev_off [B + 1]')
        if self.fx is not None and self.fx.shape != self.ev.shape:
            raise ValueError('SoundscapePlan: fx [E], one (semitones, factor) per event')
        if self.rir is not None and self.rir.shape != self.ev.shape:
            raise ValueError('SoundscapePlan: rir [E], one response index per event (-1: dry)')
        if self.target_db is not None and self.target_db.shape != self.ev.shape:
            raise ValueError('SoundscapePlan: target_db [E], one level per event')
        if self.ev_off[0] != 0 or self.ev_off[-1] != self.ev.shape[0] or bool((np.diff(self.ev_off) < 0).any()):
            raise ValueError('SoundscapePlan: ev_off is not the exclusive scan of the clips\' event counts')
        if B and int(np.diff(self.ev_off).max()) > L.SCAPE_MAXEV:
            raise ValueError(f'SoundscapePlan: a clip holds {int(np.diff(self.ev_off).max())} events, sedt_soundscape takes {L.SCAPE_MAXEV}')

    def __len__(self):
        return int(self.bg.shape[0])

    def events(self, b):
        return self.ev[int(self.ev_off[b]):int(self.ev_off[b + 1])]


def gains(ref_db, snr_db, rms):
    """float32(10^((ref_db + snr_db) / 20) / rms) from float64 arithmetic; rms == 0 (a silent background): 1.  ``rms`` is the source's
    level as an amplitude: its RMS, or 10^(L / 20) of its loudness L under level='lufs' (0 for -inf)"""
    rms = float(rms)
    if rms == 0.0:
        return np.float32(1.0)
    return np.float32(np.float64(10.0) ** ((np.float64(ref_db) + np.float64(snr_db)) / np.float64(20.0)) / np.float64(rms))


def check_bank_stats(what, sumsq, classes):
    """refuse what sedt_bank_stats found in newly staged sources: a non-finite sum of squares (a NaN or infinite sample) and a
    foreground sound (class >= 0) without energy; a silent background (class -1) is allowed"""
    for i, (q, c) in enumerate(zip(sumsq, classes)):
        if not math.isfinite(q):
            raise ValueError(f'SoundscapeClips.{what}: source {i} holds non-finite samples')
        if c >= 0 and q == 0.0:
            raise ValueError(f'SoundscapeClips.{what}: source {i} is silent: a foreground sound needs energy to be placed at an SNR')


def check_bank_loudness(what, lufs, classes):
    """refuse a foreground sound (class >= 0) at -inf LUFS - every block under the absolute gate; such a background (class -1) is allowed
    and mixed with gain 1, as a silent one is"""
    for i, (l, c) in enumerate(zip(lufs, classes)):
        if c >= 0 and l == -math.inf:
            raise ValueError(f'SoundscapeClips.{what}: source {i} lies under the absolute gate (-70 LUFS) in every block: a foreground '
                             'sound needs a loudness to be placed at an SNR')


def make_plan(backgrounds, events, rirs=None, levels=None):
    """a SoundscapePlan from hand-made records: ``backgrounds`` one entry per clip, None or (src, start, gain); ``events`` one list per
    clip of (src, cls, src_start, n, onset, gain, fade) or, with effects, (src, cls, src_start, n, onset, gain, fade, semitones,
    factor) - the plan has ``fx`` as soon as one event has the two trailing fields, the others are the identity.  Nothing but the
    shape and the event count per clip is checked here: a record outside the bank raises the clip's status on the device.
    ``rirs``: None, or one list per clip with one response index per event (-1: dry) - the plan's ``rir``.  ``levels``: None, or one
    list per clip with the level in dB / LUFS every event shall have in the clip - the plan's ``target_db``."""
    if len(backgrounds) != len(events):
        raise ValueError('make_plan: one background entry and one event list per clip')
    bg = np.zeros(len(backgrounds), BACKGROUND)
    bg['src'] = -1
    for b, g in enumerate(backgrounds):
        if g is not None:
            bg[b]['src'], bg[b]['start'], bg[b]['gain'] = int(g[0]), int(g[1]), np.float32(g[2])
    rows = [tuple(e) for clip in events for e in clip]
    if any(len(e) not in (7, 9) for e in rows):
        raise ValueError('make_plan: an event is (src, cls, src_start, n, onset, gain, fade) with an optional (semitones, factor) behind')
    ev = np.array([e[:7] for e in rows], EVENT) if rows else np.zeros(0, EVENT)
    fx = np.array([e[7:] if len(e) == 9 else (0.0, 1.0) for e in rows], FX) if any(len(e) == 9 for e in rows) else None
    off = np.concatenate([[0], np.cumsum([len(c) for c in events])]).astype(np.int64)
    if len(events) and int(np.diff(off).max()) > L.SCAPE_MAXEV:
        raise ValueError(f'make_plan: a clip holds {int(np.diff(off).max())} events, sedt_soundscape takes {L.SCAPE_MAXEV}')
    rir = None
    if rirs is not None:
        if len(rirs) != len(events) or any(len(r) != len(c) for r, c in zip(rirs, events)):
            raise ValueError('make_plan: rirs holds one list per clip, one response index per event')
        rir = np.asarray([int(i) for r in rirs for i in r], np.int32)
    target_db = None
    if levels is not None:
        if len(levels) != len(events) or any(len(l) != len(c) for l, c in zip(levels, events)):
            raise ValueError('make_plan: levels holds one list per clip, one level per event')
        target_db = np.asarray([float(v) for l in levels for v in l], np.float64)
    return SoundscapePlan(bg, ev, off.astype(np.int32), fx, rir, target_db)


def is_identity(fx):
    """bool [E]: the events whose effects are (0 semitones, factor 1) - they are not processed at all"""
    return (fx['semitones'] == 0.0) & (fx['factor'] == 1.0)


def excerpt_for(limit, factor):
    """the largest n >= 0 with floor(n factor + 0.5) <= limit, in float64 as the stage computes the length"""
    n = int(math.floor((limit + 0.5) / factor))
    while n > 0 and math.floor(n * factor + 0.5) > limit:
        n -= 1
    while math.floor((n + 1) * factor + 0.5) <= limit:
        n += 1
    return n


def draw_plan(B, lens, rms, by_class, backgrounds, window, sr, n_events=(1, 9), snr_db=(6.0, 30.0), ref_db=-30.0, max_event_seconds=None,
              fade_seconds=0.01, background=True, pitch_shift=None, time_stretch=None, reverb=None, rooms=None):
    """the plan of B soundscapes (module docstring: the order np.random is consumed in).  lens / rms: samples and float64 level per
    source as an amplitude (the RMS, or 10^(L / 20) under level='lufs'); by_class: per class the source indices of its sounds;
    backgrounds: the source indices of the background recordings; pitch_shift / time_stretch: None or the (lo, hi) range an event's
    shift in semitones / duration factor is drawn from - with both None nothing new is drawn and the plan has no ``fx``; reverb: None,
    True (every event wet) or the probability in (0, 1] that an event is wet; rooms: per room the indices of its responses"""
    wet_prob = None
    if reverb is not None and reverb is not False:
        if not rooms or any(not len(r) for r in rooms):
            raise ValueError('draw: reverb asked for, no room impulse response is staged: add_rirs() first')
        if reverb is not True:
            wet_prob = float(reverb)
            if not 0.0 < wet_prob <= 1.0:                    # (NaN fails)
                raise ValueError(f'draw: reverb {reverb!r} is neither True nor a probability in (0, 1]')
    wet_draws = reverb is not None and reverb is not False
    effects = pitch_shift is not None or time_stretch is not None
    if effects:
        from .stretch import check_effect
        p_rng = (0.0, 0.0) if pitch_shift is None else (float(pitch_shift[0]), float(pitch_shift[1]))
        f_rng = (1.0, 1.0) if time_stretch is None else (float(time_stretch[0]), float(time_stretch[1]))
        for p_, f_ in zip(p_rng, f_rng):
            check_effect(f_, p_, 'draw')
        if p_rng[0] > p_rng[1] or f_rng[0] > f_rng[1]:
            raise ValueError(f'draw: pitch_shift {pitch_shift} / time_stretch {time_stretch} is not a range lo <= hi')
    lo, hi = int(n_events[0]), int(n_events[1])
    if not 0 <= lo <= hi:
        raise ValueError(f'draw: n_events {tuple(n_events)} is not a range 0 <= lo <= hi')
    if hi > L.SCAPE_MAXEV:
        raise ValueError(f'draw: up to {hi} events per clip asked for, sedt_soundscape takes {L.SCAPE_MAXEV}')
    classes = [c for c, own in enumerate(by_class) if len(own)]
    if hi > 0 and not classes:
        raise ValueError('draw: the bank is empty: add_events() first')
    if background and not len(backgrounds):
        raise ValueError('draw: no background recording is staged: add_backgrounds() first, or background=False')
    if int(B) < 1:
        raise ValueError(f'draw: {B} clips')
    window = int(window)
    cap = window if max_event_seconds is None else max(int(round(float(max_event_seconds) * sr)), 1)
    fade = int(round(float(fade_seconds) * sr))
    bg = np.zeros(int(B), BACKGROUND)
    bg['src'] = -1
    ev, fx, rir, target_db, off = [], [], [], [], [0]
    for b in range(int(B)):
        if background:
            s = int(backgrounds[np.random.randint(len(backgrounds))])
            bg[b]['src'], bg[b]['start'], bg[b]['gain'] = s, np.random.randint(int(lens[s])), gains(ref_db, 0.0, rms[s])
        if wet_draws:
            room = rooms[np.random.randint(len(rooms))]
        for _ in range(np.random.randint(lo, hi + 1)):
            c = classes[np.random.randint(len(classes))]
            s = int(by_class[c][np.random.randint(len(by_class[c]))])
            snr = np.random.uniform(float(snr_db[0]), float(snr_db[1]))
            n = m = min(int(lens[s]), cap, window)
            if effects:
                # the effects as the plan stores them (float32), the lengths from those values as the stage computes them
                p = np.float32(0.0) if pitch_shift is None else np.float32(np.random.uniform(*p_rng))
                f = np.float32(1.0) if time_stretch is None else np.float32(np.random.uniform(*f_rng))
                p, f = np.clip(p, np.float32(p_rng[0]), np.float32(p_rng[1])), np.clip(f, np.float32(f_rng[0]), np.float32(f_rng[1]))
                n = min(int(lens[s]), excerpt_for(min(cap, window), float(f)))
                if n < 1:
                    raise ValueError(f'draw: no excerpt stretched by {float(f)} fits {min(cap, window)} samples')
                m = int(math.floor(n * float(f) + 0.5))
                fx.append((p, f))
            if wet_draws:
                wet = True if wet_prob is None else bool(np.random.uniform() < wet_prob)
                rir.append(int(room[np.random.randint(len(room))]) if wet else -1)
            src_start = np.random.randint(int(lens[s]) - n + 1)
            onset = np.random.randint(window - m + 1)
            ev.append((s, c, src_start, n, onset, gains(ref_db, snr, rms[s]), fade))
            target_db.append(np.float64(ref_db) + np.float64(snr))
        off.append(len(ev))
    return SoundscapePlan(bg, np.array(ev, EVENT) if ev else np.zeros(0, EVENT), np.asarray(off, np.int32),
                          np.array(fx, FX).reshape(-1) if effects else None, np.asarray(rir, np.int32) if wet_draws else None,
                          np.asarray(target_db, np.float64))


class SoundscapeClips(object):
    """mel: the DeviceMelSpectrogram of the model (its sample rate is the bank's after staging); labels: the class names;
    window_seconds: the clip length; max_targets: the events a clip's tables hold (1 .. 63, the stepper's TargetTables must be built
    with the same value); min_event_seconds: merged events shorter than this are dropped; collapse: merge the events of one class that
    overlap or touch, as data_utils/collapse_event.py does for the reference's corpora; peak_limit: a clip whose peak exceeds it is
    scaled down to it; level: 'rms' - ref_db and snr_db refer to the sources' RMS - or 'lufs' - to their BS.1770 loudness, measured on
    the device at staging (``lufs``, ``level_amp`` = 10^(lufs / 20) per source); stretch_n_fft: the frame length of the effects' phase
    vocoder (512, 1024 or 2048; the resampling filter is ``resample_quality``'s); reverb_n_fft: the frame length of the reverberation's
    partitioned convolution (512, 1024 or 2048); relevel: measure every event's level after its effects, on the device, before it is
    mixed (``mix``'s default; the plan needs ``target_db``).  See the module docstring."""

    STATUS_REASONS = STATUS_REASONS

    def __init__(self, mel, labels, window_seconds=10.0, max_targets=32, min_event_seconds=0.0, collapse=True, peak_limit=1.0,
                 device='cuda', resample_quality='kaiser_best', level='rms', stretch_n_fft=2048, reverb_n_fft=2048, relevel=False):
        self.mel, self.labels = mel, list(labels)
        self.window_seconds = float(window_seconds)
        self.window = int(round(self.window_seconds * mel.sr))
        self.max_targets, self.min_event_seconds = int(max_targets), float(min_event_seconds)
        self.collapse, self.peak_limit = bool(collapse), float(peak_limit)
        if not 1 <= self.max_targets <= 63:
            raise ValueError('max_targets must be in 1..63 (the target tables\' own limit)')
        if not mel.min_samples <= self.window < 2 ** 31:
            raise ValueError(f'SoundscapeClips: a window of {self.window} samples is outside {mel.min_samples} (what the front end needs) '
                             '.. 2^31 - 1')
        if math.isnan(self.min_event_seconds):
            raise ValueError('SoundscapeClips: min_event_seconds is NaN')
        if not self.peak_limit > 0.0:
            raise ValueError(f'SoundscapeClips: peak_limit {peak_limit} is not a number > 0')
        if level not in ('rms', 'lufs'):
            raise ValueError(f"SoundscapeClips: level {level!r} is neither 'rms' nor 'lufs'")
        self.level, self._loudness = level, None
        self.dev = torch.device(device)
        self.resample_quality, self._resamplers = resample_quality, {}
        self.ns, self.src_cls = [], []                      # per source: samples, class index (-1: a background recording)
        self.by_class, self.backgrounds = [[] for _ in self.labels], []
        self.rms, self.peak = np.zeros(0, np.float64), np.zeros(0, np.float32)
        self.lufs, self.level_amp = np.zeros(0, np.float64), np.zeros(0, np.float64)       # filled under level='lufs' only
        self.flat, self.src_off, self.table = None, None, None
        self.last_peak = self.last_scale = None
        self._ring, self._buf, self._amp, self._keep = None, {}, {}, []
        self.stretch_n_fft, self._stretch, self._fx_buf, self._fx_bank = int(stretch_n_fft), None, None, None
        self.last_fx = self.last_fx_status = self.last_rv_status = None
        self.reverb_n_fft, self._reverb, self.rooms, self._room_ids = int(reverb_n_fft), None, [], []
        self.relevel, self._relevel, self._relevel_out, self.last_relevel = bool(relevel), None, None, None

    # ------------------------------------------------------------------ staging
    def resampler(self, rate):
        """the DeviceResampler from ``rate`` to mel.sr, made at first use and kept"""
        rs = self._resamplers.get(int(rate))
        if rs is None:
            from .resample import DeviceResampler
            rs = self._resamplers[int(rate)] = DeviceResampler(int(rate), self.mel.sr, self.resample_quality, device=self.dev)
        return rs

    def _class_index(self, label):
        if isinstance(label, (int, np.integer)) and not isinstance(label, bool):
            if 0 <= int(label) < len(self.labels):
                return int(label)
        elif label in self.labels:
            return self.labels.index(label)
        raise ValueError(f'SoundscapeClips.add_events: class {label!r} is not one of the {len(self.labels)} labels')

    def _add(self, what, waves, classes, sample_rates):
        waves = list(waves)
        if not waves or len(waves) != len(classes):
            raise ValueError(f'SoundscapeClips.{what}: at least one source, one class per sound')
        for i, w in enumerate(waves):
            if int(w.shape[0]) == 0:
                raise ValueError(f'SoundscapeClips.{what}: source {i} is empty')
        if sample_rates is not None:
            flat, _, ns, keep = stage_resampled(waves, sample_rates, self.resampler, self.dev)
        else:
            flat, _, ns, keep = stage_recordings(waves, self.dev)
        ns = [int(n) for n in ns]
        if min(ns) < 1:
            raise ValueError(f'SoundscapeClips.{what}: source {ns.index(min(ns))} is empty')
        n_old, all_ns = len(self.ns), self.ns + ns
        joined = flat[:sum(ns)] if self.flat is None else torch.cat([self.flat[:sum(self.ns)], flat[:sum(ns)]])
        off = np.concatenate([[0], np.cumsum(all_ns)]).astype(np.int64)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        table = {'off': up(off[:-1]), 'len': up(np.asarray(all_ns, np.int64))}
        # the statistics of the new sources: one launch, read back once per add (staging is not the loop)
        sumsq = torch.zeros(len(ns), dtype=torch.float64, device=self.dev)
        peak = torch.zeros(len(ns), dtype=torch.float32, device=self.dev)
        L.check(L.load().sedt_bank_stats(L.p(joined), int(off[-1]), L.p(table['off'][n_old:]), L.p(table['len'][n_old:]), len(ns),
                                         L.p(sumsq), L.p(peak), L.stream_ptr()), 'bank_stats')
        if self.level == 'lufs':                                     # ... and their loudness: one launch more, read back with the rest
            if self._loudness is None:
                from .loudness import DeviceLoudness
                self._loudness = DeviceLoudness(self.mel.sr, self.dev)
            loud = self._loudness.launch(joined, int(off[-1]), table['off'][n_old:], table['len'][n_old:], ns)
        sumsq, peak = sumsq.cpu().numpy(), peak.cpu().numpy()
        check_bank_stats(what, sumsq, classes)
        if self.level == 'lufs':
            lufs = self._loudness.result(*loud, f'SoundscapeClips.{what}').lufs
            check_bank_loudness(what, lufs, classes)
        # everything is checked: commit
        self._keep.append(keep)                                      # the raw input lives until the copies behind it have run
        self.flat, self.src_off, self.table, self.ns = joined, off, table, all_ns
        self.src_cls = self.src_cls + list(classes)
        for i, c in enumerate(classes):
            (self.by_class[c] if c >= 0 else self.backgrounds).append(n_old + i)
        self.rms = np.concatenate([self.rms, np.sqrt(sumsq / np.asarray(ns, np.float64))])
        self.peak = np.concatenate([self.peak, peak])
        if self.level == 'lufs':
            self.lufs = np.concatenate([self.lufs, lufs])
            self.level_amp = np.concatenate([self.level_amp, np.float64(10.0) ** (lufs / np.float64(20.0))])       # (0 for -inf)
        return self

    def add_events(self, waves, event_labels, sample_rates=None):
        """stage isolated foreground sounds, each with ONE class (a name or an index): 1-D float32 / int16 at mel.sr (host or device)
        or, with ``sample_rates`` (one int or one per sound), at any rate and interleaved (frames, channels) - down-mixed and resampled
        on the device as RecordingClips.add does.  Unknown labels, empty, silent and non-finite sounds are refused, under level='lufs'
        also a sound at -inf LUFS.  Returns self."""
        classes = [self._class_index(l) for l in event_labels]
        return self._add('add_events', waves, classes, sample_rates)

    def add_backgrounds(self, waves, sample_rates=None):
        """stage background recordings (as add_events; a silent one is allowed and is mixed with gain 1).  Returns self."""
        waves = list(waves)
        return self._add('add_backgrounds', waves, [-1] * len(waves), sample_rates)

    def reverberator(self):
        """the DeviceReverb of the plans' wet events (n_fft = ``reverb_n_fft``), made at first use"""
        if self._reverb is None:
            from .reverb import DeviceReverb
            self._reverb = DeviceReverb(self.mel.sr, self.reverb_n_fft, device=self.dev, resample_quality=self.resample_quality)
        return self._reverb

    def add_rirs(self, rirs, rooms=None, sample_rates=None, normalize='energy'):
        """stage room impulse responses (DeviceReverb.add_rirs: 1-D float32 / int16 at mel.sr or, with ``sample_rates``, resampled on the
        device; normalize='energy' scales each to sum h^2 = 1).  rooms: one room id per response - a clip draws ONE room and its wet
        events draw among that room's responses; the default puts every response into one room.  Returns self."""
        rirs = list(rirs)
        ids = [0] * len(rirs) if rooms is None else list(rooms)
        if len(ids) != len(rirs):
            raise ValueError('SoundscapeClips.add_rirs: one room id per response')
        rv = self.reverberator()
        first = len(rv)
        rv.add_rirs(rirs, sample_rates=sample_rates, normalize=normalize)
        for i, room in enumerate(ids):
            if room not in self._room_ids:
                self._room_ids.append(room)
                self.rooms.append([])
            self.rooms[self._room_ids.index(room)].append(first + i)
        return self

    def __len__(self):
        return len(self.ns)

    def wave(self, src):
        """the device view of one staged source (1-D float32 at mel.sr)"""
        return self.flat[int(self.src_off[src]):int(self.src_off[src + 1])]

    # ------------------------------------------------------------------ plans
    def draw(self, B, n_events=(1, 9), snr_db=(6.0, 30.0), ref_db=-30.0, max_event_seconds=None, fade_seconds=0.01, background=True,
             pitch_shift=None, time_stretch=None, reverb=None):
        """the SoundscapePlan of B fresh soundscapes: draw_plan over the staged bank (module docstring)"""
        if not self.ns:
            raise ValueError('SoundscapeClips.draw: the bank is empty: add_events() first')
        level = self.level_amp if self.level == 'lufs' else self.rms
        return draw_plan(B, self.ns, level, self.by_class, self.backgrounds, self.window, self.mel.sr, n_events, snr_db, ref_db,
                         max_event_seconds, fade_seconds, background, pitch_shift, time_stretch, reverb, self.rooms)

    def plan(self, backgrounds, events, rirs=None, levels=None):
        """a SoundscapePlan from hand-made records (make_plan); class names in the events' second field are looked up"""
        events = [[(e[0], self._class_index(e[1]) if isinstance(e[1], str) else e[1]) + tuple(e[2:]) for e in clip] for clip in events]
        return make_plan(backgrounds, events, rirs, levels)

    # ------------------------------------------------------------------ batches
    def buffers(self, B):
        """(wave (B, window) f32, blob uint8, status int32 [B], part f32 scratch, peak f32 [B], scale f32 [B]) of batch size B, owned by
        this object and reused by every mix"""
        buf = self._buf.get(int(B))
        if buf is None:
            chunks = -(-self.window // L.SCAPE_CHUNK)
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.dev)
            buf = self._buf[int(B)] = (z((B, self.window), torch.float32), z(blob_layout(B, self.max_targets)[3], torch.uint8),
                                       z(B, torch.int32), z(B * chunks, torch.float32), z(B, torch.float32), z(B, torch.float32))
        return buf

    def stretcher(self):
        """the DeviceStretch of the plans' effects (n_fft = ``stretch_n_fft``, the filter of ``resample_quality``), made at first use"""
        if self._stretch is None:
            from .stretch import DeviceStretch
            self._stretch = DeviceStretch(self.mel.sr, self.stretch_n_fft, self.resample_quality, device=self.dev)
        return self._stretch

    def _effect_records(self, plan):
        """the host half of a plan's effects, None when every event is the identity: (the events with the transformed ones rewritten to
        (src = their own row behind the bank, src_start = 0, n = m), their SedtStretchJob records, the source table extended by one row
        per transformed event - offsets and lengths -, the samples the bank and the results take together, the workspace floats).
        A transformed event whose record does not lie inside the bank is left as it is: sedt_soundscape raises its clip's status."""
        from .stretch import stretch_jobs
        ev, n_src, ns = plan.ev, len(self.ns), np.asarray(self.ns, np.int64)
        src = np.clip(ev['src'], 0, n_src - 1)
        inside = (ev['src'] >= 0) & (ev['src'] < n_src) & (ev['src_start'] >= 0) & (ev['n'] >= 1) & (ev['src_start'] <= ns[src]) & \
            (ev['n'] <= ns[src] - ev['src_start'])
        todo = np.flatnonzero(~is_identity(plan.fx) & inside)
        if not len(todo):
            return None
        jobs, floats = stretch_jobs(ev['n'][todo], plan.fx['factor'][todo].astype(np.float64), plan.fx['semitones'][todo].astype(np.float64),
                                    self.stretch_n_fft, src_offs=self.src_off[ev['src'][todo]] + ev['src_start'][todo])
        bank = (int(self.src_off[-1]) + 3) & ~3                       # every result starts on a multiple of 4 samples behind the bank
        jobs['dst_off'] += bank
        out = ev.copy()
        out['src'][todo], out['src_start'][todo], out['n'][todo] = n_src + np.arange(len(todo)), 0, jobs['m']
        rows_off = np.concatenate([self.src_off[:-1], jobs['dst_off']]).astype(np.int64)
        rows_len = np.concatenate([ns, jobs['m']]).astype(np.int64)
        return out, jobs, rows_off, rows_len, int(jobs['dst_off'][-1] + jobs['m'][-1]), floats

    def _reverb_records(self, plan, ev, rows_off, rows_len, end):
        """the host half of a plan's reverberation, None when no event is wet.  ``ev``: the events after the stretch stage's rewrite;
        ``rows_off`` / ``rows_len``: the source table so far; ``end``: the samples the bank and the stretched rows take.  Returns a dict:
        ev - the wet events rewritten to their heads (src = the wet row, src_start 0, the same n, fade 0); bg - the clips that hold a
        wet event rewritten to (bed row, 0, 1.0); jobs (SedtReverbJob), tails, beds; the table extended by the wet rows and the bed
        rows; the samples in all; the workspace floats.  An event whose record does not lie inside the bank, and every event of a clip
        whose background record does not, is left as it is: sedt_soundscape raises the clip's status."""
        from .reverb import BED, TAIL, reverb_jobs
        rv, B, n_src = self._reverb, len(plan), len(self.ns)
        if rv is None or not len(rv):
            raise ValueError('SoundscapeClips.mix: the plan has wet events, no room impulse response is staged: add_rirs() first')
        rir = plan.rir
        if int(rir.max()) >= len(rv):
            raise ValueError(f'SoundscapeClips.mix: the plan names response {int(rir.max())}, {len(rv)} are staged')
        n_rows, ns = len(rows_len), np.asarray(self.ns, np.int64)
        src = np.clip(ev['src'], 0, n_rows - 1)
        inside = (ev['src'] >= 0) & (ev['src'] < n_rows) & (ev['src_start'] >= 0) & (ev['n'] >= 1) & (ev['onset'] >= 0) & \
            (ev['src_start'] <= rows_len[src]) & (ev['n'] <= rows_len[src] - ev['src_start'])
        g = plan.bg
        gs = np.clip(g['src'], 0, n_src - 1)
        bg_ok = (g['src'] == -1) | ((g['src'] >= 0) & (g['src'] < n_src) & (g['start'] >= 0) & (g['start'] < ns[gs]))
        clip_of = np.repeat(np.arange(B), np.diff(plan.ev_off))
        wet = np.flatnonzero((rir >= 0) & inside & bg_ok[clip_of])
        if not len(wet):
            return None
        jobs, floats = reverb_jobs(ev['n'][wet], rir[wet], rv.rir_lens, self.reverb_n_fft,
                                   src_offs=rows_off[ev['src'][wet]] + ev['src_start'][wet], fades=np.maximum(ev['fade'][wet], 0))
        jobs['dst_off'] += (int(end) + 3) & ~3                       # every wet row starts on a multiple of 4 samples behind what is there
        totals = (jobs['n'] + np.asarray(rv.rir_lens, np.int64)[jobs['rir']] - 1).astype(np.int64)
        out = ev.copy()
        out['src'][wet], out['src_start'][wet], out['fade'][wet] = n_rows + np.arange(len(wet)), 0, 0
        clips = np.unique(clip_of[wet])
        row = (self.window + 3) & ~3
        bed_off = ((int(jobs['dst_off'][-1] + totals[-1]) + 3) & ~3) + row * np.arange(len(clips), dtype=np.int64)
        tails = np.zeros(len(wet), TAIL)
        tails['wet_off'], tails['onset'], tails['head'], tails['total'], tails['gain'] = jobs['dst_off'], ev['onset'][wet], ev['n'][wet], \
            totals, ev['gain'][wet]
        beds = np.zeros(len(clips), BED)
        beds['src'], beds['start'], beds['gain'] = g['src'][clips], g['start'][clips], g['gain'][clips]
        beds['tail_lo'], beds['tail_hi'] = np.searchsorted(clip_of[wet], clips, 'left'), np.searchsorted(clip_of[wet], clips, 'right')
        beds['dst_off'] = bed_off
        bg = g.copy()
        bg['src'][clips], bg['start'][clips], bg['gain'][clips] = n_rows + len(wet) + np.arange(len(clips)), 0, np.float32(1.0)
        return dict(ev=out, bg=bg, jobs=jobs, tails=tails, beds=beds, wet=wet, clips=clips,
                    rows_off=np.concatenate([rows_off, jobs['dst_off'], bed_off]).astype(np.int64),
                    rows_len=np.concatenate([rows_len, totals, np.full(len(clips), self.window)]).astype(np.int64),
                    samples=int(bed_off[-1]) + self.window, floats=floats)

    def releveler(self):
        """the DeviceRelevel of the plans mixed with ``relevel`` (the bank's ``level``), made at first use"""
        if self._relevel is None:
            from .relevel import DeviceRelevel
            self._relevel = DeviceRelevel(self.mel.sr, self.level, device=self.dev)
        return self._relevel

    def _relevel_records(self, plan, ev, rows_off, rows_len, rvb):
        """the host half of a plan's relevel stage: (SedtRelevelJob records, the doubles of workspace), one job per valid event in plan
        order.  ``ev``: the events after the stretch and reverb stages' rewrites; ``rows_off`` / ``rows_len``: the source table they
        index; ``rvb``: _reverb_records' dict or None.  A wet event's region is its whole wet row and its gain also goes to its tail
        record; any other event's region is ev's own (src, src_start, n) - the stretched row or the bank excerpt.  An event whose
        record does not lie inside the table gets no job: sedt_soundscape raises its clip's status."""
        rl = self.releveler()
        n_rows = len(rows_len)
        src = np.clip(ev['src'], 0, n_rows - 1)
        inside = (ev['src'] >= 0) & (ev['src'] < n_rows) & (ev['src_start'] >= 0) & (ev['n'] >= 1) & (ev['src_start'] <= rows_len[src]) & \
            (ev['n'] <= rows_len[src] - ev['src_start'])
        todo = np.flatnonzero(inside)
        offs, ns = rows_off[src[todo]] + ev['src_start'][todo], ev['n'][todo].astype(np.int64)
        tail = np.full(len(todo), -1, np.int64)
        if rvb is not None:                                          # a wet event: src is its wet row, n its head; measure the whole row
            k = np.searchsorted(todo, rvb['wet'])
            ns[k], tail[k] = rows_len[ev['src'][rvb['wet']]], np.arange(len(rvb['wet']))
        return rl.jobs(offs, ns, plan.target_db[todo], ev=todo, tails=tail)

    def _effect_buffer(self, samples):
        """the f32 device buffer that holds the bank and, behind it, the transformed sounds of one batch: the bank is copied into it
        once (again after add_events / add_backgrounds, or when a batch needs more room than any before it)"""
        bank = int(self.src_off[-1])
        if self._fx_buf is None or self._fx_bank is not self.flat or self._fx_buf.numel() < samples:
            room = samples - bank
            self._fx_buf = torch.empty(bank + max(2 * room, 1 << 16), dtype=torch.float32, device=self.dev)
            self._fx_buf[:bank].copy_(self.flat[:bank])
            self._fx_bank = self.flat
        return self._fx_buf

    def mix(self, plan, status=None, relevel=None):
        """ONE sedt_soundscape call on the current stream into this object's buffers: (wave (B, window) f32 on the device, samples per
        clip - the window - as a host list, DeviceTargets).  The records travel through a ring of pinned buffers; nothing synchronises.
        A plan with effects (``fx``) runs sedt_stretch first, over its events that are not the identity: their results lie behind a
        copy of the bank in a buffer of this object's, the source table is extended by one row each, and the unchanged mixing call
        reads them as sources (``last_fx``: the jobs, the rewritten events, the buffer).  A plan without ``fx``, or with nothing but
        identities, issues the same call on the same bytes as before.
        A plan with wet events (``rir`` >= 0) then runs sedt_reverb over them - a wet event's dry input is its stretched row, or its bank
        excerpt - and sedt_reverb_bed over the clips that hold one (module docstring); the table grows by the wet rows and the bed rows,
        every record travels in the same pinned upload, and ``last_fx`` also reports the reverb jobs, tails and beds
        (``last_rv_status``: the stage's statuses).  A plan without ``rir``, or with nothing but -1, issues the calls of before.
        ``relevel`` (None: the constructor's) then issues ONE sedt_relevel launch over all valid events, behind the stretch and reverb
        stages and before sedt_reverb_bed and sedt_soundscape (module docstring): the job list travels in the same pinned upload,
        ``last_fx`` reports the jobs (``relevel_jobs``; ``ev_dev`` / ``tails_dev``: the device records the gains went to) and
        ``last_relevel`` holds the stage's (level, counts, status) on the device, in buffers of this object's that every mix reuses.  A
        plan without ``target_db`` is refused.  With relevel off the calls and the bytes are those of before.
        ``status``: an int32 [B] device tensor to raise the statuses in instead of the buffer's own (a row of a log,
        engine.train_on_recordings).  ``last_peak`` / ``last_scale`` are the clips' peaks before scaling and their scales, on the device."""
        if self.table is None:
            raise RuntimeError('SoundscapeClips.mix: add_events() / add_backgrounds() first')
        B, E = len(plan), int(plan.ev.shape[0])
        relevel = self.relevel if relevel is None else bool(relevel)
        if relevel and plan.target_db is None:
            raise ValueError('SoundscapeClips.mix: relevel asked for, the plan has no target_db: draw() fills it, plan(..., levels=) takes it')
        if relevel and not bool(np.isfinite(plan.target_db).all()):
            raise ValueError('SoundscapeClips.mix: relevel asked for, the plan\'s target_db holds a level that is not finite')
        if not 1 <= B <= L.SCAPE_MAXB:
            raise ValueError(f'SoundscapeClips.mix: 1 .. {L.SCAPE_MAXB} clips per call')
        if self._ring is None:
            self._ring = PinnedRing(self.dev)
        wave, blob, own, part, peak, scale = self.buffers(B)
        status = own if status is None else status
        if status.shape != (B,) or status.dtype != torch.int32 or not status.is_contiguous() or status.device != wave.device:
            raise ValueError('SoundscapeClips.mix: status is a contiguous int32 [B] tensor on the device')
        ev = plan.ev if E else np.zeros(1, EVENT)
        fx = self._effect_records(plan) if plan.fx is not None and E else None
        rvb = None
        if plan.rir is not None and E and bool((plan.rir >= 0).any()):
            rvb = self._reverb_records(plan, *((plan.ev, self.src_off[:-1], np.asarray(self.ns, np.int64), int(self.src_off[-1]))
                                               if fx is None else (fx[0], fx[2], fx[3], fx[4])))
        self.last_fx = self.last_relevel = None
        bg = plan.bg
        if fx is None and rvb is None:                               # no effects: the call and the bytes of a plan without ``fx`` / ``rir``
            flat, flat_len, n_src, tail = self.flat, int(self.src_off[-1]), len(self.ns), []
            rows_off, rows_len = self.src_off[:-1], np.asarray(self.ns, np.int64)
        else:
            from .stretch import JOB as STRETCH_JOB
            jobs, floats = (np.zeros(0, STRETCH_JOB), 0) if fx is None else (fx[1], fx[5])
            if fx is not None:
                ev, rows_off, rows_len, flat_len = fx[0], fx[2], fx[3], fx[4]
            if rvb is not None:
                ev, bg, rows_off, rows_len, flat_len = rvb['ev'], rvb['bg'], rvb['rows_off'], rvb['rows_len'], rvb['samples']
            flat, n_src = self._effect_buffer(flat_len), len(rows_len)
            tail = [np.zeros(-(BACKGROUND.itemsize * B + EVENT.itemsize * ev.shape[0] + 4 * (B + 1)) % 8, np.uint8),
                    rows_off.view(np.uint8), rows_len.view(np.uint8), jobs.view(np.uint8)]
            if rvb is not None:
                tail += [rvb['jobs'].view(np.uint8), rvb['tails'].view(np.uint8), rvb['beds'].view(np.uint8)]
        rl = self._relevel_records(plan, ev, rows_off, rows_len, rvb) if relevel and E else None
        if rl is not None and not len(rl[0]):
            rl = None
        extra = []
        if rl is not None:                                           # the job list behind everything else, on a multiple of 8 bytes
            head = BACKGROUND.itemsize * B + EVENT.itemsize * ev.shape[0] + 4 * (B + 1) + sum(t.size for t in tail)
            extra = [np.zeros(-head % 8, np.uint8), rl[0].view(np.uint8)]
        raw = self._ring.upload(np.concatenate([bg.view(np.uint8), ev.view(np.uint8), plan.ev_off.view(np.uint8)] + tail + extra))
        n_bg, n_ev = BACKGROUND.itemsize * B, EVENT.itemsize * ev.shape[0]
        d_bg, d_ev, d_off = raw[:n_bg], raw[n_bg:n_bg + n_ev], raw[n_bg + n_ev:n_bg + n_ev + 4 * (B + 1)]
        t_off, t_len = self.table['off'], self.table['len']
        if tail:                                                     # the stages first: their results are the sources of the rows behind the bank
            o = n_bg + n_ev + 4 * (B + 1) + tail[0].size
            t_off, t_len = raw[o:o + 8 * n_src], raw[o + 8 * n_src:o + 16 * n_src]
            o += 16 * n_src
            self.last_fx = dict(jobs=jobs, events=ev, flat=flat)
            if len(jobs):
                st = self.stretcher()
                self.last_fx_status = st.launch(flat, jobs, flat, st.workspace(floats), jobs_dev=raw[o:o + jobs.nbytes])
                self.last_fx['workspace'] = st.workspace(floats)
            o += jobs.nbytes
            if rvb is not None:
                rj, tails, beds = rvb['jobs'], rvb['tails'], rvb['beds']
                rv = self._reverb
                self.last_rv_status = rv.launch(flat, rj, flat, rv.workspace(rvb['floats']), jobs_dev=raw[o:o + rj.nbytes])
                d_tails = raw[o + rj.nbytes:o + rj.nbytes + tails.nbytes]
                d_beds = raw[o + rj.nbytes + tails.nbytes:o + rj.nbytes + tails.nbytes + beds.nbytes]
                if rl is not None:                                   # behind sedt_reverb, before the tails' gains are read
                    self._relevel_launch(flat, flat_len, rl, raw, head + extra[0].size, d_ev, ev.shape[0], d_tails, len(tails))
                L.check(L.load().sedt_reverb_bed(L.p(flat), flat_len, L.p(t_off), L.p(t_len), n_src, L.p(d_beds), len(beds), L.p(d_tails),
                                                 len(tails), self.window, L.p(flat), flat_len, L.stream_ptr()), 'reverb_bed')
                self.last_fx.update(reverb_jobs=rj, tails=tails, beds=beds, bg=bg, wet=rvb['wet'], clips=rvb['clips'],
                                    rows_off=rows_off, rows_len=rows_len, reverb_workspace=rv.workspace(rvb['floats']))
        if rl is not None and rvb is None:
            self._relevel_launch(flat, flat_len, rl, raw, head + extra[0].size, d_ev, ev.shape[0], None, 0)
        if rl is not None:
            if self.last_fx is None:
                self.last_fx = dict(events=ev, flat=flat)
            self.last_fx.update(relevel_jobs=rl[0], ev_dev=d_ev, tails_dev=d_tails if rvb is not None else None)
        L.check(L.load().sedt_soundscape(L.p(flat), flat_len, L.p(t_off), L.p(t_len), n_src, L.p(d_bg), L.p(d_ev), L.p(d_off), B,
                                         self.window, self.mel.sr, self.max_targets,
                                         self.min_event_seconds, int(self.collapse), self.peak_limit, L.p(wave), L.p(part), L.p(peak),
                                         L.p(scale), L.p(blob), L.p(status), L.stream_ptr()), 'soundscape')
        self.last_peak, self.last_scale = peak, scale
        return wave, [self.window] * B, DeviceTargets(blob, status, B, self.max_targets, ['soundscape'] * B, self.window_seconds)

    def _relevel_launch(self, flat, flat_len, rl, raw, o, d_ev, n_ev, d_tails, n_tails):
        stage, E = self.releveler(), len(rl[0])
        if self._relevel_out is None or self._relevel_out[0].shape[0] < E:          # zeroed once; a job the device refuses leaves its row
            self._relevel_out = stage.outputs(2 * E)
        out = tuple(t[:E] for t in self._relevel_out)
        self.last_relevel = stage.launch(flat, rl[0], ev=d_ev, n_ev=n_ev, tails=d_tails, n_tails=n_tails, workspace=stage.workspace(rl[1]),
                                         jobs_dev=raw[o:o + rl[0].nbytes], flat_len=flat_len, out=out)

    def batch(self, transform, plan=None, B=None, status=None, relevel=None):
        """mix -> mel -> transform: (x (B, 1, frames, n_mels), DeviceTargets).  ``plan``: a SoundscapePlan, else draw(B).  The transform
        (a DeviceBoxTransform) may augment; a DeviceViewTransform makes both views of the mean-teacher recipe and the result is
        ((x_teacher, x_student), DeviceTargets).  ``relevel``: mix's (None: the constructor's)."""
        if plan is None:
            if B is None:
                raise ValueError('SoundscapeClips.batch: plan= or B=')
            plan = self.draw(B)
        wave, lengths, targets = self.mix(plan, status=status, relevel=relevel)
        amp = self._amp.get(wave.shape[0])
        if amp is None:
            amp = self._amp[wave.shape[0]] = torch.zeros((wave.shape[0], 1 + self.window // self.mel.hop, self.mel.F), dtype=torch.float32,
                                                         device=self.dev)
        amp, nframes = self.mel(wave, lengths=lengths, out=amp)
        return transform(amp, nframes=nframes), targets
