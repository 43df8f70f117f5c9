"""Device buffers with guard bytes for the one-process kernel tests
(tests/test_interp_kernel_gpu.py, tests/test_fused_step_gpu.py), the harness
of tests/test_fold_kernel_gpu.py as a class.  Test infrastructure.

A named buffer holds GUARD bytes of FILL, `off` more bytes of FILL (the
misalignment past a 256-byte boundary), the body, and GUARD bytes of FILL.
check() compares the whole image and names the first bad element.

The control words (flags, done, ticket, err) live in one buffer, every word
or run of flag words between GUARD bytes of FILL; check_words() compares that
whole image too, so a store one word past a flag run shows.
"""
import numpy as np

GUARD, FILL = 256, 0xA5
NW = 264                      # flag words per run: 256 slices, and words after them that must not change
F0 = GUARD                    # byte offsets in the words buffer
F1 = F0 + NW * 8 + GUARD
DONE = F1 + NW * 8 + GUARD
TICKET = DONE + 8 + GUARD
ERR = TICKET + 4 + GUARD
WORDS = ERR + 4 + GUARD
FLAG_AT = {"f0": F0, "f1": F1}
DONE_INIT = 0x0123456789ABCDEF  # what *done holds before a launch: never a run number of the tests


class Rig:
    def __init__(self, hip_rt, cap):
        self.rt, self.cap, self.raws = hip_rt, cap, {}
        self.words = hip_rt.malloc(WORDS)

    def close(self):
        for p in list(self.raws.values()) + [self.words]:
            self.rt.free(p)

    def raw(self, name):
        if name not in self.raws:
            self.raws[name] = self.rt.malloc(self.cap)
        return self.raws[name]

    def place(self, name, off, body):
        """FILL, then `body` (bytes) at GUARD + off; returns the pointer to it."""
        body = np.ascontiguousarray(body).view(np.uint8)
        assert GUARD + off + body.size + GUARD <= self.cap, (name, off, body.size)
        img = np.full(GUARD + off + body.size + GUARD, FILL, np.uint8)
        img[GUARD + off:GUARD + off + body.size] = body
        self.rt.h2d(self.raw(name), img)
        return self.raw(name) + GUARD + off

    def check(self, name, off, want, what, es):
        """The whole image: guards intact, body == want; first bad element in the message."""
        want = np.ascontiguousarray(want).view(np.uint8)
        got = self.rt.d2h(self.raw(name), np.empty(GUARD + off + want.size + GUARD, np.uint8))
        img = np.full(got.size, FILL, np.uint8)
        img[GUARD + off:GUARD + off + want.size] = want
        bad = np.flatnonzero(got != img)
        if bad.size:
            b = int(bad[0]) - GUARD - off
            where = f"element {b // es}" if 0 <= b < want.size else f"guard byte {b}"
            raise AssertionError(f"{what} {name}: first bad byte {b} ({where}) got {int(got[bad[0]]):#04x} "
                                 f"want {int(img[bad[0]]):#04x}, {bad.size} bad bytes")

    @staticmethod
    def words_image(flags, done=DONE_INIT, ticket=0, err=0):
        """flags: name -> NW values."""
        img = np.full(WORDS, FILL, np.uint8)
        for name, at in FLAG_AT.items():
            img[at:at + NW * 8] = np.array([int(v) for v in flags[name]], np.uint64).view(np.uint8)
        img[DONE:DONE + 8] = np.array([done], np.uint64).view(np.uint8)
        img[TICKET:TICKET + 4] = np.array([ticket], np.uint32).view(np.uint8)
        img[ERR:ERR + 4] = np.array([err], np.uint32).view(np.uint8)
        return img

    def set_words(self, flags, done=DONE_INIT, ticket=0, err=0):
        self.rt.h2d(self.words, self.words_image(flags, done, ticket, err))

    def flag_ptr(self, name, word=0):
        return self.words + FLAG_AT[name] + 8 * word

    def check_words(self, flags, done, ticket, err, what):
        got = self.rt.d2h(self.words, np.empty(WORDS, np.uint8))
        want = self.words_image(flags, done, ticket, err)
        bad = np.flatnonzero(got != want)
        if bad.size:
            b = int(bad[0])
            where = "guard"
            for name, at in list(FLAG_AT.items()) + [("done", DONE), ("ticket", TICKET), ("err", ERR)]:
                size = NW * 8 if name in FLAG_AT else 8 if name == "done" else 4
                if at <= b < at + size:
                    w = (b - at) // 8
                    where = f"{name}[{w}]" if name in FLAG_AT else name
                    lo = at + 8 * w if size >= 8 else at
                    width = np.uint64 if size >= 8 else np.uint32
                    n = 8 if size >= 8 else 4
                    where += (f" got {int(got[lo:lo + n].view(width)[0]):#x}"
                              f" want {int(want[lo:lo + n].view(width)[0]):#x}")
            raise AssertionError(f"{what}: control words differ at byte {b} ({where}), {bad.size} bad bytes")
