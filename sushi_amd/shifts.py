"""The caller of the hot path: ``sushi.calculate_shifts`` (reference sushi.py:400-508), restated for
Python 3, plus a speculative batched form that feeds it from a few large GPU launches.

``calculate_shifts`` walks the search groups sequentially: every call of
``dst_stream.find_substream`` is centred on the shift the *previous* group committed
(sushi.py:420,432,450-452,459-462), so the reference issues 1-7 dependent searches per group.
On the GPU one search of a +-10 s window costs ~10 us of device time but a launch + readback
costs far more, so the dependent chain -- not the arithmetic -- would set the pace.

``SpeculativeStream`` breaks the chain without changing a single result.  It stands in for the
destination ``WavStream`` and answers ``find_substream`` from a cache of exact results:

* a search's answer is an absolute position in the destination stream plus the score *of that
  position*; both are independent of which window found them.  So a cached result for the same
  pattern over window W answers a request over any window W' inside W, provided the cached arg-min
  lies in W' (the first index of the minimum of a superset that falls inside the subset is the first
  index of the subset's minimum);
* on a miss the proxy runs ONE batched launch (``WavStream.find_substreams``) holding the request
  plus the searches the state machine will ask for next if the shift stays what it is now: the same
  offset and window for the following ``lookahead`` groups (full pattern; and both halves unless it
  is the small-window probe of sushi.py:431-432).

Where the shift is piecewise constant (chapters, sushi.py:120-187) that is one launch per piece.
A wrong guess costs a wasted speculative search, never a different answer: the state machine below
consumes exactly the values the sequential calls would have produced.
"""
import logging

import numpy as np

from .common import SushiError, format_time

ALLOWED_ERROR = 0.01      # sushi.py:39
SMALL_WINDOW = 1.5        # sushi.py:410


class ScriptEvent(object):
    """The part of subs.ScriptEventBase (subs.py:14-80) that calculate_shifts and the grouping code
    (sushi_amd/grouping.py) touch: a time span, a shift/diff pair, and links to another event whose shift
    it follows."""

    def __init__(self, start, end, source_index=0, text=u'', is_comment=False):
        self.source_index = source_index
        self.start = start
        self.end = end
        self.text = text
        self.is_comment = is_comment      # subs.py: AssEvent / SrtEvent attribute read by prepare_search_groups
        self._shift = 0
        self._diff = 1
        self._linked_event = None

    @property
    def linked(self):
        return self._linked_event is not None

    @property
    def shift(self):
        return self._linked_event.shift if self.linked else self._shift

    @property
    def diff(self):
        return self._linked_event.diff if self.linked else self._diff

    @property
    def duration(self):
        return self.end - self.start

    def set_shift(self, shift, audio_diff):
        assert not self.linked, 'Cannot set shift of a linked event'
        self._shift = shift
        self._diff = audio_diff

    def get_link_chain_end(self):
        return self._linked_event.get_link_chain_end() if self.linked else self

    def link_event(self, other):
        assert other.get_link_chain_end() is not self, 'Circular link detected'
        self._linked_event = other

    def resolve_link(self):
        assert self.linked, 'Cannot resolve unlinked events'
        self._shift, self._diff = self._linked_event.shift, self._linked_event.diff
        self._linked_event = None

    def __str__(self):
        return u'{0}-{1} {2}'.format(format_time(self.start), format_time(self.end), self.text)


def _span_state(group, shift=None, diff=None):
    return {"start_time": group[0].start, "end_time": group[-1].end, "shift": shift, "diff": diff}


def _log_shift(state):
    logging.info('{0}-{1}: shift: {2:0.10f}, diff: {3:0.10f}'.format(
        format_time(state["start_time"]), format_time(state["end_time"]), state["shift"], state["diff"]))


def _triple_search(dst_stream, whole, left, right, centre, window, right_offset):
    """The three searches of sushi.py:450-452 / 460-462 and their agreement test (:453 / :463)."""
    batched = getattr(dst_stream, "find_substreams", None)
    if batched is not None:
        # the three searches are independent of each other: one launch (one pass of every kernel over three searches) instead
        # of three launches one after the other -- the same three results (tools/latency.py: a triple costs ~1.1 x a single call)
        diffs, times = batched([whole, left, right], [centre, centre, centre + right_offset], [window] * 3)
        diff, whole_time, left_time, right_time = diffs[0], times[0], times[1], times[2] - right_offset
    else:
        diff, whole_time = dst_stream.find_substream(whole, centre, window)
        left_time = dst_stream.find_substream(left, centre, window)[1]
        right_time = dst_stream.find_substream(right, centre + right_offset, window)[1] - right_offset
    agree = abs(left_time - right_time) <= ALLOWED_ERROR and abs(whole_time - left_time) <= ALLOWED_ERROR
    return diff, whole_time, left_time, right_time, agree


def calculate_shifts(src_stream, dst_stream, groups_list, normal_window, max_window, rewind_thresh):
    """sushi.py:400-508.  Same arguments, same effect on the events of ``groups_list`` (set_shift /
    link_event), same log lines.  ``dst_stream`` needs ``duration_seconds`` and ``find_substream``."""
    committed, pending = [], []           # group states: settled / found but not yet trusted (:412-413)
    window = normal_window
    at = 0
    while at < len(groups_list):
        group = groups_list[at]
        whole = src_stream.get_substream(group[0].start, group[-1].end)              # :417
        t0 = group[0].start
        state = _span_state(group)
        base_shift = committed[-1]["shift"] if committed else 0                       # :420
        diff = found = None

        if not pending:
            if t0 + base_shift > dst_stream.duration_seconds:                         # :424-429
                # this and every later group starts past the end of the destination audio
                for g in groups_list[at:]:
                    committed.append(_span_state(g))
                    logging.info("{0}-{1}: outside of audio range".format(format_time(g[0].start),
                                                                          format_time(g[-1].end)))
                break
            if SMALL_WINDOW < window:                                                 # :431-432
                diff, found = dst_stream.find_substream(whole, t0 + base_shift, SMALL_WINDOW)
            if found is not None and abs((found - t0) - base_shift) <= ALLOWED_ERROR:  # :434-443
                state.update({"shift": found - t0, "diff": diff})
                committed.append(state)
                _log_shift(state)
                if window != normal_window:
                    logging.info("Going back to window {0} from {1}".format(normal_window, window))
                    window = normal_window
                at += 1
                continue

        left, right = np.split(whole, [len(whole[0]) // 2], axis=1)                   # :445 (Python 2 int division)
        right_offset = len(left[0]) / float(src_stream.sample_rate)                   # :446
        settled = False
        if t0 + base_shift < dst_stream.duration_seconds:                             # :449-455
            diff, found, lt, rt, settled = _triple_search(dst_stream, whole, left, right, t0 + base_shift,
                                                          window, right_offset)
            logging.debug('{0}-{1}: shift: {2:0.5f} [{3:0.5f}, {4:0.5f}], search offset: {5:0.6f}'.format(
                format_time(state["start_time"]), format_time(state["end_time"]), found - t0, lt - t0, rt - t0,
                base_shift))
        if not settled and pending and pending[-1]["shift"] is not None \
                and t0 + pending[-1]["shift"] < dst_stream.duration_seconds:          # :457-465
            retry_shift = pending[-1]["shift"]
            diff, found, lt, rt, settled = _triple_search(dst_stream, whole, left, right, t0 + retry_shift,
                                                          window, right_offset)
            logging.debug('{0}-{1}: shift: {2:0.5f} [{3:0.5f}, {4:0.5f}], search offset: {5:0.6f}'.format(
                format_time(state["start_time"]), format_time(state["end_time"]), found - t0, lt - t0, rt - t0,
                retry_shift))

        shift = found - t0                                                            # :467 (TypeError if nothing ran, as in the reference)
        if not settled:                                                               # :468-479
            state.update({"shift": shift, "diff": diff})
            pending.append(state)
            at += 1
            if rewind_thresh == len(pending) and window < max_window:
                logging.warning("Detected possibly broken segment starting at {0}, increasing the window from {1} "
                                "to {2}".format(format_time(pending[0]["start_time"]), window, max_window))
                window = max_window
                at = len(committed)
                del pending[:]
            continue

        if pending:                                                                   # :482-485
            logging.warning("Events from {0} to {1} will most likely be broken!".format(
                format_time(pending[0]["start_time"]), format_time(pending[-1]["end_time"])))
        pending.append(state)                                                         # :487-493
        for st in pending:
            st.update({"shift": shift, "diff": diff})
            _log_shift(st)
        committed.extend(pending)
        del pending[:]
        at += 1

    for st in pending:                                                                # :495-496
        _log_shift(st)

    for at, (group, st) in enumerate(zip(groups_list, committed + pending)):          # :498-508
        if st["shift"] is None:
            for earlier in reversed(groups_list[:at]):
                target = next((x for x in reversed(earlier) if not x.linked), None)
                if target:
                    for e in group:
                        e.link_event(target)
                    break
        else:
            for e in group:
                e.set_shift(st["shift"], st["diff"])


class SpeculativeStream(object):
    """Stands in for the destination stream inside ``calculate_shifts`` (module docstring).

    ``dst`` must offer ``find_substreams(patterns, centres, windows, with_index=True)``,
    ``_window(pattern_len, centre, window)`` -> (start_time, first sample, P) and ``sample_rate`` /
    ``duration_seconds`` (``sushi_amd.wav.WavStream`` does)."""

    def __init__(self, dst, src, groups_list, lookahead=64, max_lookahead=4096):
        self.dst = dst
        self.src = src
        self.lookahead = int(lookahead)            # groups speculated per launch; doubles while guesses hold
        self.base_lookahead = int(lookahead)
        self.max_lookahead = max(int(max_lookahead), int(lookahead))
        self._last_launch = None                   # (first group, groups speculated) of the previous launch
        self.launches = 0          # batched launches issued
        self.searches = 0          # searches computed (useful + speculative)
        self.requests = 0          # find_substream calls answered
        self.hits = 0
        self._cache = {}           # (pattern offset, length) -> [(first sample, P, abs arg-min sample, score)]
        self._groups = []          # per group: (start, whole, left, right, right_offset)
        self._role = {}            # (pattern offset, length) -> (group index, 0 whole / 1 left / 2 right)
        base = src.data.__array_interface__['data'][0]
        itemsize = src.data.itemsize
        for gi, group in enumerate(groups_list):
            whole = src.get_substream(group[0].start, group[-1].end)
            left, right = np.split(whole, [len(whole[0]) // 2], axis=1)
            right_offset = len(left[0]) / float(src.sample_rate)
            self._groups.append((group[0].start, whole, left, right, right_offset))
            for role, pat in enumerate((whole, left, right)):
                key = ((pat.__array_interface__['data'][0] - base) // itemsize, pat.shape[1])
                self._role.setdefault(key, (gi, role))
        self._src_base, self._src_itemsize = base, itemsize
        self._src_nbytes = src.data.nbytes

    # ---- what calculate_shifts reads ---------------------------------------------------------
    @property
    def duration_seconds(self):
        return self.dst.duration_seconds

    @property
    def sample_rate(self):
        return self.dst.sample_rate

    def find_substream(self, pattern, window_center, window_size):
        self.requests += 1
        key = self._key(pattern)
        if key is None:                      # not a view of the source stream: nothing to speculate on
            return self.dst.find_substream(pattern, window_center, window_size)
        start_time, first, n_pos = self.dst._window(pattern.shape[1], window_center, window_size)
        if n_pos < 1:
            raise SushiError('pattern is longer than the search window (cv2.error in the reference)')
        got = self._lookup(key, first, n_pos)
        if got is None:
            self._launch(key, pattern, window_center, window_size)
            got = self._lookup(key, first, n_pos)
        else:
            self.hits += 1
        pos, score = got
        # wav.py:188 with min_idx = pos - first
        return score, start_time + ((pos - first) / float(self.dst.sample_rate))

    # ---- internals ---------------------------------------------------------------------------
    def _key(self, pattern):
        if not isinstance(pattern, np.ndarray) or pattern.ndim != 2 or pattern.shape[0] != 1 \
                or pattern.dtype != self.src.data.dtype or pattern.strides[1] != pattern.itemsize:
            return None
        addr = pattern.__array_interface__['data'][0]
        if not (self._src_base <= addr and addr + pattern.shape[1] * pattern.itemsize <= self._src_base + self._src_nbytes):
            return None
        return ((addr - self._src_base) // self._src_itemsize, pattern.shape[1])

    def _lookup(self, key, first, n_pos):
        for (f0, p0, pos, score) in self._cache.get(key, ()):
            if f0 <= first and first + n_pos <= f0 + p0 and first <= pos < first + n_pos:
                return pos, score
        return None

    def _launch(self, key, pattern, centre, window):
        pats, centres, wins, keys = [pattern], [centre], [window], [key]
        role = self._role.get(key)
        if role is not None and self.lookahead > 0:
            gi, which = role
            # the previous guess held for every group it covered -> speculate twice as far this time;
            # it broke early (a chapter boundary, a noisy group) -> back to the base depth
            if self._last_launch is not None:
                first, count = self._last_launch
                self.lookahead = min(2 * self.lookahead, self.max_lookahead) if gi >= first + count \
                    else self.base_lookahead
            self._last_launch = (gi, min(self.lookahead, len(self._groups) - gi))
            start_g, _, _, _, roff_g = self._groups[gi]
            offset = centre - start_g - (roff_g if which == 2 else 0.0)     # the shift being probed
            probe_only = (which == 0 and window == SMALL_WINDOW)            # sushi.py:431-432 asks for nothing else
            for h in range(gi, min(gi + self.lookahead, len(self._groups))):
                start_h, whole, left, right, roff = self._groups[h]
                if start_h + offset > self.dst.duration_seconds:
                    break
                cands = [(whole, start_h + offset)] if probe_only else \
                    [(whole, start_h + offset), (left, start_h + offset), (right, start_h + offset + roff)]
                for pat, c in cands:
                    k = self._key(pat)
                    if pat.shape[1] < 1 or (k == key and c == centre):
                        continue
                    _, first, n_pos = self.dst._window(pat.shape[1], c, window)
                    if n_pos < 1 or self._lookup_window(k, first, n_pos):
                        continue
                    pats.append(pat); centres.append(c); wins.append(window); keys.append(k)
        scores, _times, positions = self.dst.find_substreams(pats, centres, wins, with_index=True)
        self.launches += 1
        self.searches += len(pats)
        for k, pat, c, w, score, pos in zip(keys, pats, centres, wins, scores, positions):
            _, first, n_pos = self.dst._window(pat.shape[1], c, w)
            self._cache.setdefault(k, []).append((first, n_pos, int(pos), score))

    def _lookup_window(self, key, first, n_pos):
        """True if some cached search of this pattern already covers [first, first + n_pos)."""
        return any(f0 <= first and first + n_pos <= f0 + p0 for (f0, p0, _, _) in self._cache.get(key, ()))


def calculate_shifts_batched(src_stream, dst_stream, groups_list, normal_window, max_window, rewind_thresh,
                             lookahead=64, max_lookahead=4096):
    """calculate_shifts with the destination stream behind a SpeculativeStream: identical results,
    a handful of batched GPU launches instead of thousands of dependent ones.  Returns the proxy
    (its counters tell how the speculation went)."""
    proxy = SpeculativeStream(dst_stream, src_stream, groups_list, lookahead=lookahead, max_lookahead=max_lookahead)
    calculate_shifts(src_stream, proxy, groups_list, normal_window, max_window, rewind_thresh)
    return proxy


def calculate_shifts_at_speed(src_stream, dst_stream, groups_list, speed, normal_window, max_window, rewind_thresh, batched=True):
    """calculate_shifts for a source that plays `speed` times as fast as the destination (sushi_amd.retime: a source instant t lies
    at t * speed on the destination's clock).  The source is put on the destination's clock (``src_stream.retimed(speed)``), every
    event gets a shadow ``ScriptEvent(start * speed, end * speed)``, and the unmodified ``calculate_shifts_batched`` (or, with
    batched=False, ``calculate_shifts``) runs on the shadows.  An original event e then gets the shift that carries it to where its
    shadow landed, ``shadow.start + shadow.shift - e.start`` (formed as shadow.shift + (shadow.start - e.start), so that speed 1
    leaves the shift as it is), and the shadow's diff; an event whose shadow was linked is linked to the original of the shadow's
    target.  With speed 1 shifts and diffs are exactly the unmodified function's.  A linked event follows its target's SHIFT, as in
    the reference; at a speed other than 1 that places it only approximately -- off by (speed - 1) * (e.start - target.start)
    from where its own shadow would lie, 0.2 s for an event 5 s from its target at 25/24 (links are made only for groups past the
    destination's end).  Returns what that function returns."""
    from .retime import as_ratio
    ratio = as_ratio(speed)
    factor = ratio.numerator / float(ratio.denominator)
    retimed = src_stream.retimed(ratio)
    original = {}
    shadow_groups = []
    for group in groups_list:
        shadows = []
        for e in group:
            sh = ScriptEvent(e.start * factor, e.end * factor, e.source_index, e.text, e.is_comment)
            original[id(sh)] = e
            shadows.append(sh)
        shadow_groups.append(shadows)
    if batched:
        result = calculate_shifts_batched(retimed, dst_stream, shadow_groups, normal_window, max_window, rewind_thresh)
    else:
        result = calculate_shifts(retimed, dst_stream, shadow_groups, normal_window, max_window, rewind_thresh)
    for shadows, group in zip(shadow_groups, groups_list):
        for sh, e in zip(shadows, group):
            if sh.linked:
                e.link_event(original[id(sh._linked_event)])
            else:
                e.set_shift(sh.shift + (sh.start - e.start), sh.diff)
    return result


def calculate_group_shifts(src_stream, dst_stream, groups, window, centre_shifts=0.0, clamp=None, capacity=None):
    """One shift per group of events, found jointly (sushi_amd.joint): `groups` is a list of lists of ScriptEvent;
    every event's pattern is src_stream.get_substream(e.start, e.end) and its centre e.start + centre_shift (centre_shifts: one
    number for all groups, or one per group).  All groups go through one dst_stream.find_joint_many call with window `window`
    (seconds).  Every event gets set_shift(centre_shift + delta, its own score at the joint shift).  SushiError for an event whose
    pattern is empty.  clamp, capacity: find_joint_many's (rows clamped at a threshold; the scores the events get stay the true ones).
    Returns the JointMatch of every group."""
    groups = [list(g) for g in groups]
    try:
        shifts = [float(s) for s in centre_shifts]
    except TypeError:
        shifts = [float(centre_shifts)] * len(groups)
    if not groups or len(shifts) != len(groups) or any(not g for g in groups):
        raise SushiError("calculate_group_shifts: non-empty groups, one centre shift per group")
    requests = []
    for group, shift in zip(groups, shifts):
        patterns = [src_stream.get_substream(e.start, e.end) for e in group]
        for e, p in zip(group, patterns):
            if p.shape[1] < 1:
                raise SushiError("calculate_group_shifts: event %s has no samples in the source" % e)
        requests.append((patterns, [e.start + shift for e in group]))
    kw = {} if clamp is None and capacity is None else dict(clamp=clamp, capacity=capacity)
    matches = dst_stream.find_joint_many(requests, [window] * len(groups), **kw)
    for group, shift, match in zip(groups, shifts, matches):
        for e, score in zip(group, match.event_scores):
            e.set_shift(shift + match.delta, score)
    return matches


def calculate_segmented_shifts(src_stream, dst_stream, events, window, penalty, centre_shift=0.0, clamp=None, capacity=None):
    """A shift per event, changing only where a change pays (sushi_amd.segments): `events` is a list of ScriptEvent
    in order; every event's pattern is src_stream.get_substream(e.start, e.end) and its centre e.start + centre_shift.  All go
    through one dst_stream.find_segments call with window `window` (seconds) and `penalty` (its docstring).  Every event gets
    set_shift(centre_shift + its delta, its own score there).  SushiError for an event whose pattern is empty.  clamp, capacity:
    find_segments' (rows clamped at a threshold; the scores the events get stay the true ones).  Returns the Segmentation."""
    events = list(events)
    shift = float(centre_shift)
    if not events:
        raise SushiError("calculate_segmented_shifts: no events")
    patterns = [src_stream.get_substream(e.start, e.end) for e in events]
    for e, p in zip(events, patterns):
        if p.shape[1] < 1:
            raise SushiError("calculate_segmented_shifts: event %s has no samples in the source" % e)
    kw = {} if clamp is None and capacity is None else dict(clamp=clamp, capacity=capacity)
    found = dst_stream.find_segments(patterns, [e.start + shift for e in events], window, penalty, **kw)
    for e, delta, score in zip(events, found.deltas, found.event_scores):
        e.set_shift(shift + delta, score)
    return found


def chapter_penalties(events, chapter_times, penalty, chapter_penalty):
    """One penalty per event for find_track / calculate_tracked_shifts: `chapter_penalty` for an event whose chapter differs from
    that of the event before it, `penalty` for every other one (event 0 gets `penalty`; its value is ignored by the pass).  Cuts
    happen at chapter marks, which is why the reference groups events by chapter: a change of shift is cheap there and dear inside a
    chapter.  chapter_times are the chapters' start points in seconds (the first one opens the first chapter and decides nothing);
    an event belongs to the chapter its END falls in -- the number of later start points below its end --, as in
    grouping.groups_from_chapters.  SushiError for a penalty that is not a finite number >= 0."""
    try:
        inside, across = float(penalty), float(chapter_penalty)
        limits = sorted(float(t) for t in list(chapter_times)[1:])
    except (TypeError, ValueError):
        raise SushiError("chapter_penalties: penalties and chapter times are numbers")
    if not (np.isfinite(inside) and inside >= 0 and np.isfinite(across) and across >= 0):
        raise SushiError("chapter_penalties: penalties must be finite and >= 0")
    chapters = [sum(1 for t in limits if e.end > t) for e in events]
    return [inside] + [across if b != a else inside for a, b in zip(chapters[:-1], chapters[1:])] if chapters else []


def calculate_tracked_shifts(src_stream, dst_stream, events, window, penalty, max_rate=None, reach=None, step_cost=0.0,
                             centre_shift=0.0, margins=False, guard=None, marginals=False, clamp=None, capacity=None, order=None,
                             wide=False):
    """A shift per event that may move a little between events and jump where a jump pays (sushi_amd.track):
    `events` is a list of ScriptEvent in order; every event's pattern is src_stream.get_substream(e.start, e.end) and its centre
    e.start + centre_shift.  All go through one dst_stream.find_track call with window `window` (seconds), `penalty`, and max_rate
    or reach and step_cost (its docstring).  Every event gets set_shift(centre_shift + its delta, its own score there).  SushiError
    for an event whose pattern is empty.  margins, guard and marginals are find_track's: with margins=True the Track also says how
    firmly every event is placed (event_margin, event_alt_delta, ...).  clamp, capacity: find_track's (rows clamped at a threshold;
    the scores the events get stay the true ones).  order: find_track's (None; True: the events are kept in order in the
    destination; or one back per event), and `penalty` may be one number per event (chapter_penalties gives them from chapter marks):
    either takes the ordered pass, whose margins are calculate_ordered_shifts'.  wide: find_track's (a reach up to
    32767 samples where step_cost is 0: a long stretch without an event no longer ends the call).  Returns the
    Track."""
    events = list(events)
    shift = float(centre_shift)
    if not events:
        raise SushiError("calculate_tracked_shifts: no events")
    patterns = [src_stream.get_substream(e.start, e.end) for e in events]
    for e, p in zip(events, patterns):
        if p.shape[1] < 1:
            raise SushiError("calculate_tracked_shifts: event %s has no samples in the source" % e)
    # (the keywords a caller did not use are not passed on: a stream without them still serves)
    more = {} if clamp is None and capacity is None else dict(clamp=clamp, capacity=capacity)
    if order is not None:
        more["order"] = order
    if wide:
        more["wide"] = True
    found = dst_stream.find_track(patterns, [e.start + shift for e in events], window, penalty, max_rate=max_rate, reach=reach,
                                  step_cost=step_cost, margins=margins, guard=guard, marginals=marginals, **more)
    for e, delta, score in zip(events, found.deltas, found.event_scores):
        e.set_shift(shift + delta, score)
    return found


def calculate_ordered_shifts(src_stream, dst_stream, events, window, penalty, order=True, max_rate=None, reach=None, step_cost=0.0,
                             centre_shift=0.0, margins=False, guard=None, marginals=False, clamp=None, capacity=None):
    """calculate_tracked_shifts through dst_stream.find_ordered_track (its docstring): the events are kept
    in order in the destination (order: True, the default here; None; or one back per event), `penalty` may be one number per event,
    and with margins=True the Track says how firmly the ordered pass places every event (guard, marginals: find_ordered_track's).
    Every event gets set_shift(centre_shift + its delta, its own score there).  Returns the Track."""
    return _ordered_shifts("calculate_ordered_shifts", dst_stream.find_ordered_track, src_stream, events, window, penalty, order, max_rate,
                           reach, step_cost, centre_shift, margins, guard, marginals, clamp, capacity)


def calculate_ordered_wide_shifts(src_stream, dst_stream, events, window, penalty, order=True, max_rate=None, reach=None, step_cost=0.0,
                                  centre_shift=0.0, margins=False, guard=None, marginals=False, clamp=None, capacity=None):
    """calculate_ordered_shifts through dst_stream.find_ordered_wide_track (its docstring): a reach may be up to 32767
    samples where step_cost is 0, so one long stretch without an event does not end the call.  Everything else is
    calculate_ordered_shifts'.  Returns the Track."""
    return _ordered_shifts("calculate_ordered_wide_shifts", dst_stream.find_ordered_wide_track, src_stream, events, window, penalty, order,
                           max_rate, reach, step_cost, centre_shift, margins, guard, marginals, clamp, capacity)


def _ordered_shifts(name, find, src_stream, events, window, penalty, order, max_rate, reach, step_cost, centre_shift, margins, guard,
                    marginals, clamp, capacity):
    events = list(events)
    shift = float(centre_shift)
    if not events:
        raise SushiError("%s: no events" % name)
    patterns = [src_stream.get_substream(e.start, e.end) for e in events]
    for e, p in zip(events, patterns):
        if p.shape[1] < 1:
            raise SushiError("%s: event %s has no samples in the source" % (name, e))
    found = find(patterns, [e.start + shift for e in events], window, penalty, order=order, max_rate=max_rate, reach=reach,
                 step_cost=step_cost, margins=margins, guard=guard, marginals=marginals,
                 **({} if clamp is None and capacity is None else dict(clamp=clamp, capacity=capacity)))
    for e, delta, score in zip(events, found.deltas, found.event_scores):
        e.set_shift(shift + delta, score)
    return found


def calculate_drifting_shifts(src_stream, dst_stream, events, window, max_rate, centre_shift=0.0, resolution=1.0, clamp=None,
                              capacity=None):
    """A shift per event along one line of shifts (sushi_amd.drift): `events` is a list of ScriptEvent; every
    event's pattern is src_stream.get_substream(e.start, e.end) and its centre e.start + centre_shift.  All go through one
    dst_stream.find_drift call with window `window` (seconds), rates out to +-max_rate and `resolution` (its docstring).  Every
    event gets set_shift(centre_shift + its event_delta, its own score there).  SushiError for an event whose pattern is empty.
    clamp, capacity: find_drift's (rows clamped at a threshold; the scores the events get stay the true ones).  Returns the
    DriftMatch."""
    events = list(events)
    shift = float(centre_shift)
    if not events:
        raise SushiError("calculate_drifting_shifts: no events")
    patterns = [src_stream.get_substream(e.start, e.end) for e in events]
    for e, p in zip(events, patterns):
        if p.shape[1] < 1:
            raise SushiError("calculate_drifting_shifts: event %s has no samples in the source" % e)
    kw = {} if clamp is None and capacity is None else dict(clamp=clamp, capacity=capacity)
    found = dst_stream.find_drift(patterns, [e.start + shift for e in events], window, max_rate, resolution=resolution, **kw)
    for e, delta, score in zip(events, found.event_deltas, found.event_scores):
        e.set_shift(shift + delta, score)
    return found
