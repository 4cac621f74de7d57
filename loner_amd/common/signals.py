"""Signals and slots for a single process: the interface of src/common/signals.py that Tracker uses (register, emit, has_value,
get_value, flush), written afresh.  A Signal is a channel; every registered Slot receives its own deep copy of each emitted value,
first in first out.  Tracker is duck-typed on these members, so the reference's multi-process signals work in their place."""
import collections
import copy


class StopSignal:
    """Emitted in place of data to tell a listener to stop."""


class Slot:
    def __init__(self):
        self._items = collections.deque()

    def has_value(self) -> bool:
        return len(self._items) > 0

    def get_value(self):
        """The oldest value, or None when there is none."""
        return self._items.popleft() if self._items else None

    def __len__(self):
        return len(self._items)

    def _insert(self, value):
        self._items.append(copy.deepcopy(value))


class Signal:
    def __init__(self, synchronous: bool = False, single_process: bool = True):
        if synchronous or not single_process:
            raise NotImplementedError("loner_amd.common.signals is single-process and asynchronous; use the reference's signals "
                                      "across processes")
        self._slots = []

    def register(self) -> Slot:
        self._slots.append(Slot())
        return self._slots[-1]

    def emit(self, value) -> None:
        for slot in self._slots:
            slot._insert(value)

    def flush(self) -> None:
        """Drops whatever the listeners have not taken."""
        leftover = sum(len(slot) for slot in self._slots)
        if leftover:
            print(f"Warning: {leftover} leftover items in the queues")
        for slot in self._slots:
            slot._items.clear()
