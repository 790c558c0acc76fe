"""The host side of a recorder's record log (hipims_mi._RecordLog, behind Domain.probes_* and Domain.zones_*) without a GPU: which
of the records read back from a full device buffer survive a state_restore.  The library is replaced by a dozen lines that keep
the device buffer as a list of rows; every expectation is the plain list of the rows sampled, never the helper's own output.
Capacity 3, stride 2: the smallest shape that drains more than once and leaves a partly filled buffer behind."""
import numpy as np
import pytest

from hipims_mi import _RecordLog

CAPACITY, STRIDE = 3, 2


class FakeRecorder:
    """What the library does for a recorder: a buffer of CAPACITY rows, counted, read and emptied on request.  `history`: every
    row sampled, for restore()."""

    def __init__(self, dtype, first=0):
        self.rows, self.history, self.first = [], [], first
        self.log = _RecordLog(dtype, lambda: (len(self.rows), CAPACITY, STRIDE), self.read, self.rows.clear)
        self.log.opened()

    def read(self, out):
        out[:] = self.rows

    def sample(self):
        """Domain.*_sample: the helper first, then the library's sample (which refuses a full buffer).  -> the row taken"""
        self.log.before_sample()
        assert len(self.rows) < CAPACITY
        row = [self.first + 2 * len(self.history), self.first + 2 * len(self.history) + 1]
        self.rows.append(row)
        self.history.append(row)
        return row

    def restore(self, n, taken):
        """hp_state_restore to a state saved after `taken` samples: the library reports n records again, the last n of them."""
        del self.history[taken:]
        self.rows[:] = self.history[taken - n:]


@pytest.fixture(params=[np.float64, np.uint64], ids=["float64", "uint64"])
def dtype(request):
    return request.param


def same(log, rows, dtype):
    rec = log.records()
    assert rec.dtype == dtype and rec.shape == (len(rows), STRIDE)
    assert rec.tolist() == [[dtype(v) for v in row] for row in rows]


def test_eight_samples_drain_twice_and_come_back_in_order(dtype):
    fake = FakeRecorder(dtype)
    rows = [fake.sample() for _ in range(8)]
    assert [len(a) for a in fake.log.drained] == [3, 3]
    same(fake.log, rows, dtype)
    assert fake.log.info() == dict(samples=8, pending=2, capacity=CAPACITY, stride=STRIDE)


@pytest.mark.parametrize("reported", [1, 0])
def test_restore_keeps_the_drained_records_the_checkpoint_had(dtype, reported):
    """`reported`: the library's count after the restore -- the saved one, or 0 where it finds that the buffer was reset (drained)
    after the checkpoint.  Either way the records are those of the checkpoint."""
    fake = FakeRecorder(dtype)
    rows = [fake.sample() for _ in range(4)]               # one drain, one pending
    assert fake.log.info()["pending"] == 1
    fake.log.saved()
    for _ in range(4):
        fake.sample()
    assert [len(a) for a in fake.log.drained] == [3, 3]
    fake.restore(reported, 4)
    fake.log.restored()
    same(fake.log, rows, dtype)
    rows += [fake.sample() for _ in range(4)]
    straight = FakeRecorder(dtype)                         # a run without the save and the restore
    assert rows == [straight.sample() for _ in range(8)]
    same(fake.log, rows, dtype)
    same(straight.log, rows, dtype)
    assert fake.log.info()["samples"] == straight.log.info()["samples"] == 8      # (how many of them are pending depends on `reported`)


def test_restore_to_a_checkpoint_taken_before_the_first_drain(dtype):
    fake = FakeRecorder(dtype)
    rows = [fake.sample() for _ in range(3)]               # everything still in the device buffer
    fake.log.saved()
    fake.sample()                                          # drains
    assert [len(a) for a in fake.log.drained] == [3]
    fake.restore(3, 3)
    fake.log.restored()
    assert fake.log.drained == []
    same(fake.log, rows, dtype)


def test_a_checkpoint_of_another_generation_counts_for_nothing(dtype):
    fake = FakeRecorder(dtype)
    for _ in range(4):
        fake.sample()
    fake.log.saved()
    fake.log.closed()
    fake.rows.clear()
    fake.log.opened()
    for _ in range(5):
        fake.sample()
    assert [len(a) for a in fake.log.drained] == [3]
    fake.restore(0, 4)                                     # the library finds no count of this epoch: 0
    fake.log.restored()
    assert fake.log.drained == [] and fake.log.info()["samples"] == 0
    same(fake.log, [], dtype)


def test_reset_forgets_everything_and_a_closed_log_does_nothing():
    fake = FakeRecorder(np.uint64)
    for _ in range(5):
        fake.sample()
    fake.log.saved()
    fake.log.reset()
    assert fake.log.drained == [] and fake.rows == [] and fake.log.info()["samples"] == 0
    fake.sample()
    fake.restore(0, 5)
    fake.log.restored()                                    # the reset began another generation
    assert fake.log.info()["samples"] == 0
    fake.log.closed()
    fake.log.saved()
    assert fake.log.saved_at is None
    fake.log.restored()
    fake.log.before_sample()                               # (the library's own answer follows in Domain.*_sample)
    assert fake.log.drained == []


def test_a_word_above_2_to_the_63_comes_back_exactly():
    big = 2 ** 63 + 1
    fake = FakeRecorder(np.uint64, first=big)
    rows = [fake.sample() for _ in range(4)]
    assert rows[0][0] == big
    rec = fake.log.records()
    assert rec.dtype == np.uint64 and [[int(v) for v in row] for row in rec] == rows
