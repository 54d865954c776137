"""Per-phase timing of the persistent decoder kernels from shader-clock stamps (library built with -DASR_DP_TRACE in
scratchlibs/lib_trace.so): mean cycles between marks over decoder steps 8..15 of workgroup (group 0, slice 0)."""
import ctypes, sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, ROOT + '/semi-supervised-asr_amd']
import torch, numpy as np
import hip_backend as hb
dev = torch.device('cuda')
B, Tp, L, D, E, C, K, V = 32, 100, 101, 512, 128, 10, 100, 34
A = O = D; KX = D + O + E
g = torch.Generator().manual_seed(5)
rnd = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(dev)
buf = hb.DecBuffers(B, Tp, A, D, O, E, C, K, L, True, dev, True)
s0 = 1.0 / np.sqrt(D)
buf.P.copy_(rnd(B, Tp, A, sc=0.5)); buf.Q.copy_(rnd(B, Tp, O, sc=0.5)); buf.wcat.copy_(rnd(4 * D, KX, sc=s0))
buf.bcat.copy_(rnd(4 * D, sc=s0)); buf.convw.copy_(rnd(C, 2 * K + 1, sc=0.1)); buf.gvec.copy_(rnd(A, sc=s0))
watt = rnd(A, C, sc=0.3); buf.wattT.copy_(watt.t()); buf.w0.fill_(1.0 / Tp)
buf.xmask.copy_((torch.rand(L, B, O + E, generator=g) > 0.3).float().to(dev) / 0.7)
buf.X.zero_(); buf.X[:L, :, D + O:] = rnd(L, B, E, sc=0.5)
buf.Xd.zero_(); buf.Xd[:L, :, D + O:] = buf.X[:L, :, D + O:] * buf.xmask[:, :, O:]
wdec = rnd(A, D, sc=s0)
buf.bind(bo=rnd(O, sc=s0), wdec=wdec, watt=watt)
buf.zbuf.zero_(); buf.dws.zero_()
buf.acc["G"][1:, :, :D + O] = rnd(L, B, D + O, sc=0.01)
buf.wcatT.copy_(buf.wcat.t()); buf.wdecT.copy_(wdec.t())
fs = buf.fwd_struct(); bs = buf.bwd_struct(with_dws=False)
xch, ctrl = hb.persist_scratch(dev, trace=True)
st = hb.stream()
l = ctypes.CDLL(ROOT + '/scratchlibs/lib_trace.so')
l.asr_dec_seq_fwd_persist.argtypes = [ctypes.POINTER(hb.DecFwd), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
l.asr_dec_seq_bwd_persist.argtypes = [ctypes.POINTER(hb.DecBwd), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
X, C_ = ctypes.c_void_p(xch.data_ptr()), ctypes.c_void_p(ctrl.data_ptr())
def report(name, nmarks):
    t = ctrl[32:32 + 8 * 16 * 2].cpu().numpy().view(np.int64).reshape(8, 16)[:, :nmarks]
    dl = np.diff(t, axis=1).mean(0)
    step = (t[1:, 0] - t[:-1, 0]).mean()
    print(name, 'cycles/step %.0f' % step, ' deltas:', ' '.join('%d:%.0f' % (i + 1, x) for i, x in enumerate(dl)))
for _ in range(2):
    ctrl.zero_()
    assert l.asr_dec_seq_fwd_persist(ctypes.byref(fs), X, C_, st) == 0
    torch.cuda.synchronize(); report('fwd', 11)
for _ in range(2):
    ctrl.zero_()
    assert l.asr_dec_seq_bwd_persist(ctypes.byref(bs), hb.ptr(buf.Mf), X, C_, st) == 0
    torch.cuda.synchronize(); report('bwd', 10)
    t = ctrl[32:32 + 8 * 16 * 2].cpu().numpy().view(np.int64).reshape(8, 16)
    print('   (e) split: df+barrier %.0f | dwext %.0f | dconv %.0f | prefetchA %.0f' % ((t[:, 10] - t[:, 4]).mean(), (t[:, 11] - t[:, 10]).mean(), (t[:, 12] - t[:, 11]).mean(), (t[:, 5] - t[:, 12]).mean()))
