"""Stream schedule shared by the model classes: the online teacher's iteration runs on its own HIP stream.

The teacher's step and the student's forward / teacher-independent loss terms have no data dependence, so they are
enqueued on two streams; the student's stream joins the teacher's where the teacher's features are first read, and the
teacher's stream is released by an event recorded at the last main-stream launch that reads its buffers.  The many small
layers of the two networks, which cannot fill 256 CUs alone, overlap; the arithmetic is unchanged.
``model.serialize_streams = True`` (set_stream_schedule(False), used by bench.py's profiled steps and by the tests'
references) keeps everything on one stream.

Every launch is enqueued from the calling host thread; the launch-bound models' answer to host overhead is gcc_amd.replay
(the iteration re-issued from native code)."""
import torch

from .. import ops

# The multi-stream schedule's tile plan (pair split, weight-gradient workgroup targets: big / 128 x 128).  The library's defaults
# (256 / 512) are for a launch that has the chip to itself; on the weight-gradient side stream of the production schedule half of
# that is faster end to end (+0.6 %, profiles/r02_ab_tables.md r03w / r03x; re-measured: profiles/r3l_ab_plans.txt)
_PRODUCTION_PLAN = (0, 128, 256)

class TeacherStreamMixin:
    def _ensure_plan(self):
        """state THIS model's tile plan (pair split, halo columns, weight-gradient split targets) for the launches the calling
        thread is about to enqueue: ops.set_plan -- thread-local host state that travels with every convolution call
        (gcc_conv_t.plan); the library itself holds no plan any more (round 5)."""
        plan = getattr(self, '_plan', None)
        if plan is None:
            return
        pair, wgs_big, wgs = plan[:3]
        ops.set_plan(pair=max(pair, 0), halo_hc=1 if pair == 1 else 0, wgrad_wgs_big=max(wgs_big, 0), wgrad_wgs=max(wgs, 0))

    def restore_library_plan(self):
        """back to the library's default plan on this thread (model teardown / tests that go on to call the kernels directly)"""
        self._plan = None
        ops.set_plan()

    def set_stream_schedule(self, concurrent, plan=None):
        """concurrent=True: the production schedule (student, online teacher, auxiliary and weight-gradient streams).
        False: every launch on one stream.  plan: the library's tile plan -- 'production' (what the multi-stream schedule runs:
        no pair split, half-chip weight-gradient splits) or 'alone' (for launches that have the chip to themselves:
        the pair split, full-chip weight-gradient splits); default: 'production' with concurrent streams, 'alone' without.
        bench.py times one single-stream step under each plan (a launch's duration is then the kernel's own)."""
        from .. import engine
        self.serialize_streams = not concurrent
        if getattr(self, 'teacher_model', None) is not None:
            self.teacher_model.serialize_streams = not concurrent
        engine.OVERLAP_WGRAD = bool(concurrent) and engine.overlap_wgrad_default(getattr(self, '_world', 1))
        if plan is None:
            plan = 'production' if concurrent else 'alone'
        assert plan in ('production', 'alone')
        self._plan = _PRODUCTION_PLAN if plan == 'production' else (1, -1, -1)
        if getattr(self, 'teacher_model', None) is not None:
            self.teacher_model._plan = self._plan
        self._ensure_plan()

    def _teacher_stream(self):
        self._ensure_plan()
        if getattr(self, 'serialize_streams', False):
            return False
        if getattr(self, '_tstream', None) is None:
            self._tstream = torch.cuda.Stream(device=self.device)
            if getattr(self, '_plan', None) is None:
                self._plan = _PRODUCTION_PLAN
                self._ensure_plan()
        return self._tstream

    def _mark_teacher_free(self):
        """main stream: no later launch reads the teacher's buffers -- its stream may move on from here"""
        ev = getattr(self, '_teacher_free', None)
        if ev is None:
            ev = self._teacher_free = ops.Event()      # re-recorded: the teacher's wait holds the record it saw
        ev.record()

    def _note_input(self, input):
        """set_input(): order this stream -- and, through _release_teacher_stream, the teacher's -- behind whatever produced
        a device-resident batch.  A batch dict may carry 'ready' (a torch.cuda.Event recorded by its producer after the last
        kernel that wrote its tensors: gcc_amd.data's loaders and bench.py set it); without one, device tensors are assumed
        to have been produced on the stream set_input is called on, and an event recorded here stands for them (the
        teacher then also waits for everything else already enqueued on this stream).  Host tensors need nothing: the
        H2D copy is issued on the consuming stream itself.  The tensors are marked as used on this stream so that the
        caching allocator does not hand their memory to the producer's stream while the copies below are still pending."""
        ev = input.get('ready') if hasattr(input, 'get') else None
        dev = [v for v in input.values() if torch.is_tensor(v) and v.is_cuda] if hasattr(input, 'values') else []
        if dev:
            cur = ops.current_stream()
            if ev is not None:
                ops.wait_event(cur, ev)
            else:
                ev = getattr(self, '_own_input_event', None)
                if ev is None:
                    ev = self._own_input_event = ops.Event()
                ev.record(cur)
            for t in dev:
                t.record_stream(cur)
        self._input_ready = ev if dev else None

    def _release_teacher_stream(self, ts):
        ev = getattr(self, '_teacher_free', None)
        if ev is not None:
            ops.wait_event(ts, ev)
        else:
            ops.wait_stream(ts, ops.current_stream())
        # the batch the teacher is about to read (set_input on its own stream) must exist: ADVICE r1, race on a
        # device-resident batch written by main-stream kernels after _teacher_free was recorded
        ready = getattr(self, '_input_ready', None)
        if ready is not None:
            ops.wait_event(ts, ready)

    def _run_teacher(self, fn):
        """run fn() (teacher work) on the teacher's stream if there is one; returns the stream (or False)"""
        ts = self._teacher_stream()
        if ts:
            self._release_teacher_stream(ts)
            with ops.on_stream(ts):
                fn()
        else:
            fn()
        return ts

    def _aux_stream(self):
        """second stream of the student: work that does not depend on the generator's output (the discriminator's pass
        over the real pair) runs here next to the generator's forward"""
        if getattr(self, 'serialize_streams', False) or not torch.cuda.is_available():
            return False
        if getattr(self, '_astream', None) is None:
            self._astream = torch.cuda.Stream(device=self.device)
        return self._astream

    @staticmethod
    def _join(ts):
        if ts:
            ops.wait_stream(ops.current_stream(), ts)

