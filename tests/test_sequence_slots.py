"""Sequence mode's ring arithmetic (dodt_amd.pipeline.sequence_slots) against a small model of the order in which
FramePairPipeline.push_frame() enqueues a sequence on its four streams, and the argument checks; no GPU.

The model keeps, per enqueued piece of work, a vector clock over the streams: an event wait merges the clock of the
work waited for.  A ring is deep enough when every reader of a slot is ordered behind the slot's writer of the same
keyframe and in front of its next writer -- by stream order or by a wait that exists when the later one is enqueued."""
import pytest

from dodt_amd import config
from dodt_amd.pipeline import FramePairPipeline, IMG_RING, POINT_RING, PREP_RING, sequence_slots

STREAMS = ('main', 'img', 'c0', 'c1')      # BEV stack; image stack; frame 0's and frame 1's side stream


class Model(object):
    """push_frame()'s enqueue order, with the slots sequence_slots() gives at the depths under test."""

    def __init__(self, **depths):
        self.depths = depths
        self.ops = []                              # dict(stream, index, clock, name, reads, writes)
        self.last = {s: None for s in STREAMS}     # the stream's last piece of work
        self.marks = {}                            # (stream, mark name) -> the work a mark was recorded behind
        self.step, self.prepped, self.pending = 0, -1, None
        self.primed, self.sequence = False, 0

    def slots(self, k):
        return sequence_slots(k, **self.depths)

    def key(self, k):
        """Keyframe k of the running sequence (a new sequence's first frame takes the slots of the last one's last)."""
        return (self.sequence, k)

    def op(self, stream, name, waits=(), reads=(), writes=()):
        prev = self.last[stream]
        clock = dict(prev['clock']) if prev else {s: 0 for s in STREAMS}
        for w in waits:
            if w is not None:
                for s in STREAMS:
                    clock[s] = max(clock[s], w['clock'][s])
        clock[stream] = (prev['index'] if prev else 0) + 1
        o = dict(stream=stream, index=clock[stream], clock=clock, name=name, reads=tuple(reads), writes=tuple(writes))
        self.ops.append(o)
        self.last[stream] = o
        return o

    # -- the pieces of a call, in push_frame()'s order ----------------------------------------------------------------
    def prep_new(self, k):
        """Keyframe k + 1 as frame 1 of step k, on c1 behind everything c0 holds so far."""
        s = self.slots(k)
        o = self.op('c1', 'prep new %d' % (k + 1), waits=[self.last['c0']],
                    writes=[('prep', s.prep[1], self.key(k + 1)), ('points', s.points[1], self.key(k + 1))])
        self.marks['c1', 'prep', k % 3] = o

    def prep(self, k, ahead):
        conv = [self.marks.get((s, 'conv', k & 1)) for s in ('main', 'img')] if ahead and k >= 2 else []
        o = self.op('c0', 'prep carried %d' % k, waits=conv + [self.marks['c1', 'prep', (k - 1) % 3]],
                    reads=[('points', self.slots(k).points[0], self.key(k))])
        self.marks['c0', 'prep', k % 3] = o
        if conv:
            self.op('c1', 'wait convs', waits=conv)
        self.prep_new(k)
        self.prepped = k

    def image_forward(self, k, waits):
        o = self.op('img', 'image forward %d' % (k + 1), waits=waits, writes=[('img', self.slots(k).img[1], self.key(k + 1))])
        self.marks['img', 'conv', k & 1] = o

    def tail(self, k):
        s = self.slots(k)
        conv = [self.marks['main', 'conv', k & 1], self.marks['img', 'conv', k & 1]]
        return [self.op(c, 'tail %d frame %d' % (k, f), waits=conv,
                        reads=[('img', s.img[f], self.key(k + f)), ('prep', s.prep[f], self.key(k + f))])
                for f, c in enumerate(('c0', 'c1'))]

    def push(self, lookahead):
        k = self.step
        if not self.primed:
            self.prep_new(k - 1)
            self.image_forward(k - 1, [self.marks['c1', 'prep', (k - 1) % 3], self.last['c0']])
            self.primed = True
            if lookahead:
                self.prep(k, ahead=True)
            return
        if self.prepped != k:
            self.prep(k, ahead=False)
        preps = [self.marks[c, 'prep', k % 3] for c in ('c0', 'c1')]
        self.marks['main', 'conv', k & 1] = self.op('main', 'bev stack %d' % k, waits=preps)
        self.image_forward(k, preps)
        if lookahead:
            self.prep(k + 1, ahead=True)
        if self.pending is not None:
            ends = self.tail(self.pending)
            self.op('main', 'wait tails', waits=ends)
            self.op('img', 'wait tails', waits=ends)
        self.pending = k
        self.step += 1

    def finish(self):
        if self.pending is not None:
            ends = self.tail(self.pending)
            self.op('main', 'join', waits=ends + [self.last['img']])
            self.pending = None

    def end_sequence(self):
        self.primed, self.prepped, self.sequence = False, -1, self.sequence + 1

    # -- the check ------------------------------------------------------------------------------------------------------
    def collisions(self):
        """(ring, slot, reader, writer) of every read of a slot that is not ordered behind the write of its own
        keyframe, or not in front of a later keyframe's write of the same slot."""
        def before(a, b):
            return b['clock'][a['stream']] >= a['index']
        bad = []
        for r in self.ops:
            for ring, slot, key in r['reads']:
                for w in self.ops:
                    for wring, wslot, wkey in w['writes']:
                        if (wring, wslot) != (ring, slot):
                            continue
                        if (wkey == key and not before(w, r)) or (wkey > key and not before(r, w)):
                            bad.append((ring, slot, r['name'], w['name']))
        return bad


def _drive(model, steps, lookahead, finish_every=0):
    model.push(lookahead)                          # primes
    for i in range(steps):
        model.push(lookahead and i + 1 < steps)
        if finish_every and (i + 1) % finish_every == 0:
            model.finish()                         # (a look-ahead may stand announced behind it)
    model.finish()
    return model.collisions()


def test_slots_follow_the_keyframe():
    """Frame f of step k is keyframe k + f: frame 1's slots of step k are frame 0's of step k + 1, in every ring."""
    assert (IMG_RING, PREP_RING, POINT_RING) == (3, 4, 3)
    for k in range(40):
        a, b = sequence_slots(k), sequence_slots(k + 1)
        for ring, depth in zip(('img', 'prep', 'points'), (IMG_RING, PREP_RING, POINT_RING)):
            assert getattr(a, ring)[1] == getattr(b, ring)[0] == (k + 1) % depth
            assert getattr(a, ring)[0] != getattr(a, ring)[1]


@pytest.mark.parametrize('finish_every', [0, 1, 3])
@pytest.mark.parametrize('lookahead', [False, True])
def test_no_slot_is_written_under_a_reader(lookahead, finish_every):
    assert _drive(Model(), 14, lookahead, finish_every) == []


@pytest.mark.parametrize('lookahead', [False, True])
def test_a_second_sequence_primes_over_the_first(lookahead):
    m = Model()
    assert _drive(m, 12, lookahead) == []
    m.end_sequence()
    assert _drive(m, 12, lookahead) == []


@pytest.mark.parametrize('lookahead', [False, True])
def test_two_image_slots_collide(lookahead):
    """The tail of step k is enqueued behind the image forward of the call for step k + 1, which with two slots writes
    the slot that tail's frame 0 reads."""
    bad = _drive(Model(img_ring=2), 12, lookahead)
    assert bad and {b[0] for b in bad} == {'img'}
    assert ('img', 1, 'tail 1 frame 0', 'image forward 3') in bad


def test_three_prep_sets_collide_under_lookahead():
    """Pair mode's depth: the look-ahead prep enqueued in the call for step k + 2 writes keyframe k + 4's set in front
    of the tail of step k + 1, whose frame 0 reads keyframe k + 1's -- the same set of three.  Without look-ahead three hold."""
    bad = _drive(Model(prep_ring=3), 12, True)
    assert bad and {b[0] for b in bad} == {'prep'}
    assert ('prep', 1, 'tail 1 frame 0', 'prep new 4') in bad
    assert _drive(Model(prep_ring=3), 12, False) == []


def test_the_model_sees_a_missing_wait():
    """The new frame's prep runs on frame 1's stream, the last reader of its slots (the carried frame's tail) on
    frame 0's: without the wait between them the model reports it, so its silence above means something."""
    class NoWait(Model):
        def prep_new(self, k):
            s = self.slots(k)
            self.marks['c1', 'prep', k % 3] = self.op(
                'c1', 'prep new %d' % (k + 1), writes=[('prep', s.prep[1], self.key(k + 1)), ('points', s.points[1], self.key(k + 1))])
    assert _drive(NoWait(), 12, True) != []


def test_argument_checks():
    with pytest.raises(ValueError, match='sequence'):
        FramePairPipeline(None, config.PYRAMID_DODT, None, None, pairs_per_step=2, sequence=True)
    assert config.CARS_EXAMPLE['frames_per_sample'] == 1
    with pytest.raises(ValueError, match='sequence'):
        FramePairPipeline(None, config.CARS_EXAMPLE, None, None, sequence=True)
    # (the refusals come first in each call: a pipeline that was never built shows them)
    seq, plain = object.__new__(FramePairPipeline), object.__new__(FramePairPipeline)
    seq.sequence, plain.sequence = True, False
    with pytest.raises(ValueError, match='push_frame'):
        seq.run(None, None, None)
    with pytest.raises(ValueError, match='push_frame_from_host'):
        seq.run_from_host(None, None, None)
    with pytest.raises(ValueError, match='sequence=True'):
        plain.push_frame(None, 0, None)
    with pytest.raises(ValueError, match='sequence=True'):
        plain.push_frame_from_host(None, 0, None)
