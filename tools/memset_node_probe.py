"""Does a memset node of a captured graph zero its range on every replay?  No project code: the runtime's
hipMemsetAsync captured on a torch side stream, a torch kernel after it, the range poisoned between replays."""
import ctypes
import torch

hip = ctypes.CDLL("libamdhip64.so")
hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
hip.hipMemsetAsync.restype = ctypes.c_int
for words in (576, 60000):
    buf = torch.empty(words, dtype=torch.int64, device="cuda")
    other = torch.empty(words, dtype=torch.int64, device="cuda")
    src = torch.arange(1 << 20, device="cuda")
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rc = hip.hipMemsetAsync(buf.data_ptr(), 0, words * 8, side.cuda_stream)
            buf.add_(1)
            rc2 = hip.hipMemsetAsync(other.data_ptr(), 0, words * 8, side.cuda_stream)
            other.add_(2)
    torch.cuda.synchronize()
    for i in range(4):
        if i:
            dst.copy_(src)
        buf.fill_(-123456789)
        other.fill_(-123456789)
        g.replay()
        torch.cuda.synchronize()
        u, v = buf.unique(), other.unique()
        print(f"memset probe words={words} replay {i + 1}: rc={rc},{rc2} distinct values {[hex(x & (2**64 - 1)) for x in u.tolist()[:4]]} "
              f"{[hex(x & (2**64 - 1)) for x in v.tolist()[:4]]}", flush=True)
