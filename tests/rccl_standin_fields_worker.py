"""Worker of tests/test_gpu_fields_slabs.py: soda_hip_run_slab_fields (the C slab driver
for programs over several fields) with `world` ranks as host threads of THIS process on
the one GPU, over the test-only librccl stand-in (tests/rccl_standin).  No torch here: the
stand-in must be the first object with soname librccl.so in the process.  Runs every case
of a JSON list [app, dims, world, iterate, wanted exchange, max_depth] in turn; the inputs
come from an .npz per case (in_<name>), each rank's own rows of every output go to
case<i>.rank<r>.npz."""
import ctypes
import json
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soda-compiler_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)


def main():
  standin_path, cases_path, out_dir = sys.argv[1:4]
  standin = ctypes.CDLL(standin_path, mode=ctypes.RTLD_GLOBAL)
  from soda_hip import frontend
  from soda_hip.codegen import spec as specmod
  from soda_hip.runtime import capi, host
  hip = ctypes.CDLL('libamdhip64.so')
  lib = capi.lib()
  for index, (app, dims, world, iterate, wanted, max_depth) in enumerate(
      json.load(open(cases_path))):
    sample = os.path.join(ROOT, 'tests', 'samples', app + '.soda')
    if not os.path.exists(sample):
      sample = os.path.join(ROOT, 'tests', 'samples', 'extra', app + '.soda')
    spec = specmod.spec_from_stencil(frontend.load(sample))
    blob = os.path.join(ROOT, 'soda-compiler_amd', 'blobs', app + '.hsaco')
    data = np.load(os.path.join(out_dir, 'case%d.in.npz' % index))
    full = [data['in_' + t['name']] for t in spec['inputs']]
    n = len(full)
    shape = full[0].shape
    rows = dims[-1]
    # the reach: the hull over the fields of one iteration's margins
    r_lo, r_hi = spec['radius']['lo'][-1], spec['radius']['hi'][-1]
    exchange = ctypes.c_int(min(wanted, iterate))
    capi.check(lib.soda_hip_slab_exchange(rows, world, r_lo, r_hi, wanted,
                                          ctypes.byref(exchange)))
    comms = (ctypes.c_void_p * world)()
    if world > 1:
      assert standin.ncclCommInitAll(comms, world, None) == 0
    base, extra = divmod(rows, world)
    errors, results = [None] * world, [None] * world
    abort_lock = threading.Lock()

    def abort_all():
      with abort_lock:
        for r in range(world):
          if comms[r]:
            standin.ncclCommAbort(ctypes.c_void_p(comms[r]))
            comms[r] = None

    def rank_main(rank):
      try:
        prog = host.open_program(blob=blob, spec=spec)   # one plan per host thread
        prog.set_max_depth(max_depth)
        stream = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
        hull = prog.margins(1)
        assert (hull[0][-1], hull[1][-1]) == (r_lo, r_hi)
        slab = capi.Slab()
        slab.rank, slab.world = rank, world
        slab.reach_lo, slab.reach_hi = r_lo, r_hi
        slab.exchange = exchange.value
        slab.order, slab.cut = capi.SLAB_SERIAL, capi.SLAB_CUT_STATIC
        for d, v in enumerate(dims):
          slab.dims[d] = v
        slab.own_first = rank * base + min(rank, extra)
        slab.own_last = slab.own_first + base + (1 if rank < extra else 0)
        local = (ctypes.c_int64 * 4)()
        g_lo, res_first, res_last, res_at = (ctypes.c_int64() for _ in range(4))
        capi.check(lib.soda_hip_slab_layout(
            prog.handle, ctypes.byref(slab), iterate, local, ctypes.byref(g_lo),
            ctypes.byref(res_first), ctypes.byref(res_last), ctypes.byref(res_at)))
        assert (res_first.value, res_last.value) == (slab.own_first, slab.own_last)
        # the re-cut and the bands-first order are refused before anything is sent
        for field, value, text in (('cut', capi.SLAB_CUT_RECUT, 'static cut only'),
                                   ('order', capi.SLAB_BANDS_FIRST, 'serial order only')):
          bad = capi.Slab.from_buffer_copy(slab)
          setattr(bad, field, value)
          one = (ctypes.c_void_p * n)(*[1] * n)
          rc = lib.soda_hip_run_slab_fields(prog.handle, ctypes.byref(bad), comms[rank], one,
                                            one, one, iterate, stream, one, None)
          assert rc == -8 and text in lib.soda_hip_last_error().decode(), (field, rc)
        local_shape = (local[len(dims) - 1],) + shape[1:]
        own = slab.own_last - slab.own_first
        levels = []
        for level in range(3):
          arrays = []
          for j in range(n):
            dt = full[j].dtype
            arr = host.DeviceArray(int(np.prod(local_shape)) * dt.itemsize)
            # rows nobody filled hold a pattern no sweep produces
            fill = np.full(local_shape, 0x7f, dtype=np.uint8).repeat(dt.itemsize).view(dt) \
                .reshape(local_shape)
            if level == 0:
              fill[g_lo.value:g_lo.value + own] = full[j][slab.own_first:slab.own_last]
            arr.upload(fill)
            arrays.append(arr)
          levels.append(arrays)
        capi.check(lib.soda_hip_stream_synchronize(None))
        ptrs = [(ctypes.c_void_p * n)(*[a.ptr for a in arrays]) for arrays in levels]
        result = (ctypes.c_void_p * n)()
        count = ctypes.c_int()
        rc = lib.soda_hip_run_slab_fields(
            prog.handle, ctypes.byref(slab), comms[rank], ptrs[0], ptrs[1], ptrs[2], iterate,
            stream, result, ctypes.byref(count))
        if rc:
          message = lib.soda_hip_last_error().decode()
          lib.soda_hip_stream_synchronize(stream)
          raise RuntimeError('soda_hip_run_slab_fields: %d %s' % (rc, message))
        capi.check(lib.soda_hip_stream_synchronize(stream))
        outs = []
        for j in range(n):
          which = [lv[j] for lv in levels[1:] if lv[j].ptr == result[j]]
          assert len(which) == 1, 'result %d is neither b nor c' % j
          out = which[0].download(local_shape, full[j].dtype)
          outs.append(out[res_at.value:res_at.value + own].copy())
        # a is never written by a sweep: its own rows are the input still
        for j in range(n):
          back = levels[0][j].download(local_shape, full[j].dtype)
          assert np.array_equal(back[g_lo.value:g_lo.value + own].view(np.uint8),
                                full[j][slab.own_first:slab.own_last].view(np.uint8))
        results[rank] = (slab.own_first, slab.own_last, count.value, outs)
        for arrays in levels:
          for arr in arrays:
            arr.free()
        prog.close()
      except BaseException as e:   # noqa: BLE001 - reported by the parent
        errors[rank] = e
        abort_all()      # peers blocked in the exchange must not hang

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
      t.start()
    for t in threads:
      t.join(timeout=120)
    if any(t.is_alive() for t in threads):
      print('case %d: a rank is still blocked after 120 s' % index, file=sys.stderr)
      os._exit(3)
    for rank, e in enumerate(errors):
      if e is not None:
        print('case %d rank %d: %r' % (index, rank, e), file=sys.stderr)
    if any(e is not None for e in errors):
      sys.exit(2)
    messages, nbytes = ctypes.c_longlong(), ctypes.c_longlong()
    if world > 1:
      standin.rccl_standin_traffic(ctypes.c_void_p(comms[0]), ctypes.byref(messages),
                                   ctypes.byref(nbytes))
    for rank, (first, last, count, outs) in enumerate(results):
      np.savez(os.path.join(out_dir, 'case%d.rank%d.npz' % (index, rank)),
               **{'out%d' % j: o for j, o in enumerate(outs)})
      with open(os.path.join(out_dir, 'case%d.rank%d.json' % (index, rank)), 'w') as f:
        json.dump(dict(first=first, last=last, exchange=exchange.value, exchanges=count,
                       messages=messages.value, bytes=nbytes.value), f)
    for c in comms:
      if c:
        standin.ncclCommDestroy(ctypes.c_void_p(c))


if __name__ == '__main__':
  main()
