"""Time single decoder-step kernels in a dependent chain (L launches) for ablated builds in scratchlibs/."""
import sys, os, ctypes, glob
ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0]=[ROOT, ROOT+'/semi-supervised-asr_amd']
import torch, hip_backend as hb
dev=torch.device('cuda')
B,Tp,A,D,O,E,C,K,L=32,100,512,512,512,128,10,100,101
def noise(buf):
    for v in vars(buf).values():
        if torch.is_tensor(v): v.normal_(0,0.1)
buf=hb.DecBuffers(B,Tp,A,D,O,E,C,K,L,False,dev,False)
noise(buf)
buf.w0.fill_(1.0/Tp)
bo=torch.zeros(O,device=dev); wdec=torch.randn(A,D,device=dev)*0.04; watt=torch.randn(A,C,device=dev)*0.3
buf.bind(bo=bo,wdec=wdec,watt=watt)
fs=buf.fwd_struct()
st=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
for path in sorted(glob.glob(ROOT+'/scratchlibs/lib_*.so')):
    l=ctypes.CDLL(path); l.asr_dec_seq_fwd.restype=ctypes.c_int
    l.asr_dec_seq_fwd.argtypes=[ctypes.POINTER(hb.DecFwd),ctypes.c_int,ctypes.c_int,ctypes.c_void_p]
    best=1e9
    for r in range(3):
        torch.cuda.synchronize(); e0=torch.cuda.Event(enable_timing=True); e1=torch.cuda.Event(enable_timing=True)
        e0.record(); rc=l.asr_dec_seq_fwd(ctypes.byref(fs),0,L,st); e1.record(); torch.cuda.synchronize()
        assert rc==0, rc
        best=min(best,e0.elapsed_time(e1)*1e3/L)
    print('%-20s %.2f us/launch'%(os.path.basename(path),best),flush=True)

# ---- backward kernels (libs named lib_b*)
bufb=hb.DecBuffers(B,Tp,A,D,O,E,C,K,L,False,dev,True)
noise(bufb)
bufb.bind(bo=bo,wdec=wdec,watt=watt)
bufb.ws.copy_(torch.softmax(torch.randn(L,B,Tp,device=dev),-1))
bs=bufb.bwd_struct(with_dws=False)
for path in sorted(glob.glob(ROOT+'/scratchlibs/libb_*.so')):
    l=ctypes.CDLL(path); l.asr_dec_seq_bwd.restype=ctypes.c_int
    l.asr_dec_seq_bwd.argtypes=[ctypes.POINTER(hb.DecBwd),ctypes.c_int,ctypes.c_int,ctypes.c_void_p]
    best=1e9
    for r in range(3):
        torch.cuda.synchronize(); e0=torch.cuda.Event(enable_timing=True); e1=torch.cuda.Event(enable_timing=True)
        e0.record(); rc=l.asr_dec_seq_bwd(ctypes.byref(bs),0,L,st); e1.record(); torch.cuda.synchronize()
        assert rc==0, rc
        best=min(best,e0.elapsed_time(e1)*1e3/L)
    print('%-20s %.2f us/launch'%(os.path.basename(path),best),flush=True)
