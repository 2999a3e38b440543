// gi_pool.h -- the path pool of the streaming pipeline: its field arrays, PathRef, PathPool, the named moves (pool_begin, load, store), the queue
// append of a wave (wave_append) and the slot -> sample rule (sample_of).  Device side only.
// Needs gi_device.h (PathRec, Ray) and gi_layout.h (kPoolRecordBytes); included by gi_kernels.hip ahead of gi_pixels.inc, gi_stages.inc and gi_bake.inc.
//
// The streaming passes run the same per-path stage_* code as the megakernel, so both give the same numbers.
// The streaming pipeline's paths in flight: ONE ARRAY PER GROUP OF FIELDS that a stage reads or writes together, instead of one 224-byte PathRec per
// path.  A stage wants 40 - 160 bytes of a path; out of records it moved whole DRAM pages for them (exp/aos_bench.hip: the shade stage's
// read-104-write-172 pattern costs 48 ms per 477 M records as 224-byte structures, 24 ms as field arrays).  pool[slot] gives a PathRef -- the field
// names of PathRec as references -- so the stage functions (templates on the path type) read and write exactly the fields they did.
struct alignas(16) PoolRay  { double o[3], d[3]; uint32_t stream; int32_t depth; uint32_t pad_[2]; };   // 64 B: all a new path consists of, all the trace stage reads
struct alignas(16) PoolHit  { double hpos[3], hu, hv; int32_t htri; uint32_t mf; };                     // 48 B: what the trace stage leaves for the shade stage
struct alignas(16) PoolThru { double T[3], contrib[3]; };                                               // 48 B
struct alignas(16) PoolGath { double gdir[3], gcoef[3]; };                                              // 48 B: the pending photon gather (and minUV between trace and shade)
struct PathRef {
    double (&o)[3]; double (&d)[3]; uint32_t& stream; int32_t& depth; int32_t& htri; uint32_t& pad;
    double (&T)[3]; double (&contrib)[3]; double (&gdir)[3]; double (&gcoef)[3]; double (&hpos)[3]; double& hu; double& hv; double (&L)[3];
};
#define GI_POOL_BYTES_PER_SLOT (sizeof(PoolRay) + sizeof(PoolHit) + sizeof(PoolThru) + sizeof(PoolGath) + 24)
static_assert(GI_POOL_BYTES_PER_SLOT == kPoolRecordBytes, "the pool budget (gi_layout.h: plan_pool) counts this record");
struct PathPool {
    PoolRay* ray; PoolHit* hit; PoolThru* thru; PoolGath* gath; double* L;
    __device__ __forceinline__ PathRef operator[](size_t s) const
    {
        return PathRef{ray[s].o, ray[s].d, ray[s].stream, ray[s].depth, hit[s].htri, hit[s].mf, thru[s].T, thru[s].contrib, gath[s].gdir, gath[s].gcoef,
                       hit[s].hpos, hit[s].hu, hit[s].hv, *reinterpret_cast<double (*)[3]>(L + s * 3)};
    }
    __device__ __forceinline__ PathRec load(size_t s) const     // a copy in registers (finisher)
    {
        PathRec p;
        const PathRef r = (*this)[s];
        for (int k = 0; k < 3; k++) { p.o[k] = r.o[k]; p.d[k] = r.d[k]; p.T[k] = r.T[k]; p.contrib[k] = r.contrib[k]; p.gdir[k] = r.gdir[k]; p.gcoef[k] = r.gcoef[k]; p.hpos[k] = r.hpos[k]; p.L[k] = r.L[k]; }
        p.stream = r.stream; p.depth = r.depth; p.htri = r.htri; p.pad = r.pad; p.hu = r.hu; p.hv = r.hv;
        return p;
    }
    __device__ __forceinline__ void store(size_t s, const PathRec& p) const
    {
        const PathRef r = (*this)[s];
        for (int k = 0; k < 3; k++) { r.o[k] = p.o[k]; r.d[k] = p.d[k]; r.T[k] = p.T[k]; r.contrib[k] = p.contrib[k]; r.gdir[k] = p.gdir[k]; r.gcoef[k] = p.gcoef[k]; r.hpos[k] = p.hpos[k]; r.L[k] = p.L[k]; }
        r.stream = p.stream; r.depth = p.depth; r.htri = p.htri; r.pad = p.pad; r.hu = p.hu; r.hv = p.hv;
    }
};
__device__ __forceinline__ void pool_begin(const PathPool& pool, size_t slot, const Ray& ray, uint32_t sample)   // a new path: one 64-byte store (path_begin_lean)
{
    PoolRay r;
    r.o[0] = ray.o.x; r.o[1] = ray.o.y; r.o[2] = ray.o.z;
    r.d[0] = ray.d.x; r.d[1] = ray.d.y; r.d[2] = ray.d.z;
    r.stream = sample; r.depth = 0; r.pad_[0] = 0u; r.pad_[1] = 0u;
    pool.ray[slot] = r;
}
__device__ __forceinline__ uint32_t wave_append(unsigned int* counter, bool pred)
{
    const unsigned long long mask = __ballot(pred);
    if (mask == 0ull) return 0u;
    const int lane = (int)(threadIdx.x & 63u);
    const int leader = __ffsll((long long)mask) - 1;
    unsigned int base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned int)__popcll(mask));
    base = (unsigned int)__shfl((int)base, leader);
    return base + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
}

// Which sample a slot of the path pool carries.  The table slot_sample[slot] says so in general (slots are handed on from path to path).  When the
// pool holds every sample of a chunk at once, the trace stage's first pass gives item i slot i and sample sample0 + i and no slot is ever reissued:
// the table would be the identity plus sample0, so the host passes no table (nullptr, wave-uniform) and nobody writes or reads one (stream_samples).
__device__ __forceinline__ unsigned long long sample_of(const unsigned long long* slot_sample, unsigned long long sample0, uint32_t slot)
{
    return slot_sample ? slot_sample[slot] : sample0 + slot;
}
