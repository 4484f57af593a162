"""TEST INFRASTRUCTURE: one canonical line per entry of the step-plan grid for a given build of the library - status, message,
the vmapstep_describe_plan fields, the workspace bytes and the counts offset.  Two builds make the same plans exactly when their
outputs are equal (tests/test_step_plan.py keeps a reduced table of these lines; profiles/step_plan_refactor.txt the digests of the
full one).

    python tests/tools/step_plan_dump.py LIBRARY [--reduced] [--digest]
"""
import ctypes
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vmap_amd import _lib  # noqa: E402

N_OBJ = (1, 7, 8, 9, 20, 32, 50, 256, 257)
RAYS = (1, 12, 120, 150, 256, 300, 600, 1200, 4800)
SAMPLES = (1, 10, 14, 32, 33, 64, 65, 96, 128, 129)
HIDDEN = (16, 32, 48, 64, 96, 128, 256, 288)
WEIGHTS = (0, 1, 3)                                    # 3: not a weight_dtype
MAX_STEPS = (1, 20, 256, 257)
# (workgroups_per_object, kernel, generic_finalize, ws_flags), None = no tuning struct at all
TUNINGS = ((None,) + tuple((0, k, 0, 0) for k in (1, 2, 3, 4, 5, 6, 7, 8, 17, -1)) + tuple((w, 0, 0, 0) for w in (1, 2, 50, 1000))
           + tuple((0, 0, 0, f) for f in (1, 2, 4, 8)) + ((50, 0, 0, 2), (0, 0, 1, 0)))

FULL = dict(n_obj=N_OBJ, rays=RAYS, samples=SAMPLES, hidden=HIDDEN, weights=WEIGHTS, tunings=TUNINGS, max_steps=MAX_STEPS)
# the recorded table: every width, family and refusal the full grid reaches, at the shapes the plan rules turn on
REDUCED = dict(n_obj=(1, 9), rays=(12, 1200), samples=(10, 33), hidden=(32, 64, 128, 256), weights=(0,),
               tunings=(None, (0, 1, 0, 0), (0, 2, 0, 0), (0, 5, 0, 0), (0, 6, 0, 0), (0, 8, 0, 0), (50, 0, 0, 2), (0, 0, 0, 8)), max_steps=(20,))
REDUCED_EXTRA = ((1, 1200, 14, 128, 0, None, 257), (20, 120, 10, 32, 3, None, 20), (1, 100, 14, 256, 0, None, 1), (1, 4800, 14, 256, 0, None, 256),
                 (50, 120, 10, 32, 1, None, 1), (50, 120, 10, 32, 1, (0, 8, 0, 0), 1), (1, 120, 10, 48, 0, None, 20), (1, 120, 65, 128, 0, None, 20),
                 (1, 120, 129, 96, 0, None, 20), (0, 120, 10, 32, 0, None, 20), (1, 120, 10, 32, 0, (0, 7, 0, 0), 20), (1, 120, 10, 32, 0, None, 0),
                 (256, 256, 10, 64, 1, None, 20), (1, 600, 14, 128, 0, None, 20), (1, 150, 14, 128, 0, (0, 0, 0, 1), 20), (1, 1200, 14, 128, 0, (0, 0, 0, 4), 20),
                 (3, 50, 12, 96, 0, (2, 0, 0, 0), 20), (1, 100, 40, 256, 0, None, 20), (20, 120, 10, 32, 0, (0, 4, 0, 0), 20), (20, 120, 10, 32, 0, (0, 0, 1, 0), 20),
                 (257, 12, 10, 32, 0, None, 20), (257, 1200, 10, 64, 0, None, 20), (257, 1200, 10, 128, 0, None, 20), (257, 12, 10, 256, 0, None, 20))


def entries(grid, extra=()):
    """(n_obj, rays, samples, hidden, weight_dtype, tuning, max_steps) of every grid entry"""
    yield from itertools.product(grid["n_obj"], grid["rays"], grid["samples"], grid["hidden"], grid["weights"], grid["tunings"], grid["max_steps"])
    yield from extra


class Asker:
    """The three plan queries of one build of the library for one entry."""

    def __init__(self, library):
        self.lib = _lib.load(library)
        self.info, self.nbytes, self.counts = _lib.PlanInfo(), ctypes.c_size_t(), ctypes.c_size_t()
        self.fields = [k for k, _ in _lib.PlanInfo._fields_[1:]]

    def __call__(self, e):
        """-> (status, message, kernel, the describe_plan integers ..., workspace bytes, counts offset); the three calls must agree on
        the status, which the returned one is"""
        lib = self.lib
        sh = _lib.Shape(*e[:5])
        if e[5] is not None:
            t = _lib.Tuning(*e[5])
            sh.tuning = ctypes.pointer(t)
        rc = lib.vmapstep_describe_plan(ctypes.byref(sh), e[6], ctypes.byref(self.info))
        if rc:
            msg = lib.vmapstep_last_error().decode()
            rb = lib.vmapstep_workspace_bytes(ctypes.byref(sh), e[6], ctypes.byref(self.nbytes))
            mb = lib.vmapstep_last_error().decode()
            rk = lib.vmapstep_workspace_counts_offset(ctypes.byref(sh), e[6], ctypes.byref(self.counts))
            assert (rb, mb, rk, lib.vmapstep_last_error().decode()) == (rc, msg, rc, msg), e
            return (rc, msg)
        assert lib.vmapstep_workspace_bytes(ctypes.byref(sh), e[6], ctypes.byref(self.nbytes)) == 0, e
        assert lib.vmapstep_workspace_counts_offset(ctypes.byref(sh), e[6], ctypes.byref(self.counts)) == 0, e
        info = self.info
        return (0, "", info.kernel.decode()) + tuple(getattr(info, k) for k in self.fields) + (self.nbytes.value, self.counts.value)


def line(e, answer):
    return " ".join(str(x) for x in e[:5]) + " " + ("-" if e[5] is None else ",".join(str(x) for x in e[5])) + f" {e[6]} | " + \
        " | ".join(str(x) for x in answer)


def main(argv):
    ask = Asker(argv[0])
    grid, extra = (REDUCED, REDUCED_EXTRA) if "--reduced" in argv else (FULL, ())
    digest, n = hashlib.sha256(), 0
    for e in entries(grid, extra):
        text = line(e, ask(e)) + "\n"
        digest.update(text.encode())
        n += 1
        if "--digest" not in argv:
            sys.stdout.write(text)
    if "--digest" in argv:
        print(f"{n} lines sha256 {digest.hexdigest()}")


if __name__ == "__main__":
    main(sys.argv[1:])
