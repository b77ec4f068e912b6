// MultiGpuSorter.cs — ComputeBufferSorter over the GPUs of LbvhContext.Devices (BASELINE configs[3]): one native call,
// lbvh_sort_pairs_sharded, sorts (key, value) pairs whose blocks live on different contexts — the key-range sharded sort
// (every context sorts its block, four MSD rounds of digit histograms pick the splitters, one exchange of key ranges into
// the destinations' buffers over peer-mapped memory, every destination sorts what it received).  Twin of host.py /
// lbvh_host.hpp MultiGpuSorter.  No reference counterpart: the reference sorts on one device (ComputeBufferSorter.cs:100-126).
//
// Block r = the first counts[r] pairs of keys[r] / values[r] (buffers created while rank r was current, so they live on
// rank r's context).  Sort() leaves rank q's slice of the globally sorted sequence in outKeys[q] / outValues[q] (Replicate:
// the whole sequence on every rank, the layout of a replicated tree build) and returns the slice lengths; the inputs come
// back locally sorted.  Work enqueued afterwards on rank q's context sees its outputs complete; the call blocks the host once.
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public class MultiGpuSorter : IDisposable
{
    readonly NativeBuffer[] _keys, _values, _outKeys, _outValues;

    public bool Replicate = false;

    public MultiGpuSorter(NativeBuffer[] keys, NativeBuffer[] values, NativeBuffer[] outKeys, NativeBuffer[] outValues)
    {
        int n = keys.Length;
        if (n < 1 || n > LbvhNative.SORT_SHARDED_MAX_CONTEXTS || values.Length != n || outKeys.Length != n || outValues.Length != n)
            throw new ArgumentException("MultiGpuSorter: 1 .. 16 ranks, one buffer of each kind per rank");
        for (int r = 0; r < n; r++)
            if (values[r].Context != keys[r].Context || outKeys[r].Context != keys[r].Context || outValues[r].Context != keys[r].Context)
                throw new ArgumentException("MultiGpuSorter: rank " + r + "'s buffers live on different contexts");
        _keys = keys;
        _values = values;
        _outKeys = outKeys;
        _outValues = outValues;
    }

    public uint[] Sort(uint[] counts)
    {
        int n = _keys.Length;
        if (counts.Length != n) throw new ArgumentException("MultiGpuSorter.Sort: one count per rank");
        var ctxs = new IntPtr[n];
        var k = new IntPtr[n];
        var v = new IntPtr[n];
        var ok = new IntPtr[n];
        var ov = new IntPtr[n];
        var cap = new uint[n];
        for (int r = 0; r < n; r++)
        {
            if (counts[r] > (uint)Math.Min(_keys[r].count, _values[r].count))
                throw new ArgumentException("MultiGpuSorter.Sort: rank " + r + "'s count exceeds its buffers");
            ctxs[r] = _keys[r].Context;
            k[r] = _keys[r].Pointer;
            v[r] = _values[r].Pointer;
            ok[r] = _outKeys[r].Pointer;
            ov[r] = _outValues[r].Pointer;
            cap[r] = (uint)Math.Min(_outKeys[r].count, _outValues[r].count);
        }
        var sliceCounts = new uint[n];
        LbvhNative.Check(ctxs[0], LbvhNative.lbvh_sort_pairs_sharded(ctxs, (uint)n, k, v, counts, ok, ov, cap, sliceCounts,
                                                                     Replicate ? LbvhNative.SORT_SHARDED_REPLICATE : 0u));
        return sliceCounts;
    }

    public void Dispose()
    {
        // nothing of its own to free: the buffers belong to the caller, the scratch to the native contexts
    }
}
