"""engine.Handle.close at interpreter shutdown: a module-level Context that keeps a course log is collected after the modules'
globals were set to None.  close() must not need them: a handle left set behind a destroy that ran is destroyed a second time
by __del__ (a double free in the library)."""
import ctypes

from reina_model_amd import engine as eng


class _Owner(eng.Handle):
    DESTROY = 'destroy'

    def __init__(self, destroyed, inner=None):
        self.f = {'destroy': lambda h: destroyed.append(h.value)}
        self.inner = inner
        self._h = ctypes.c_void_p(5 if inner is None else 7)

    def _closing(self):
        if self.inner is not None:
            self.inner.close()


def test_close_destroys_once_when_the_modules_globals_are_gone(monkeypatch):
    destroyed = []
    course = _Owner(destroyed)
    log = _Owner(destroyed, inner=course)          # (as a DeviceLog closes its DeviceCourse first)
    monkeypatch.setattr(eng, 'ctypes', None)       # what the interpreter leaves of a module's globals at shutdown
    log.__del__()
    course.__del__()
    log.close()
    assert destroyed == [5, 7] and not log._h and not course._h


def test_close_is_idempotent_and_a_closed_handle_is_null():
    destroyed = []
    h = _Owner(destroyed)
    h.close()
    h.close()
    assert destroyed == [5] and not h._h and isinstance(h._h, ctypes.c_void_p) and h._h.value is None
