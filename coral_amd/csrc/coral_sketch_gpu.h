// coral_sketch_gpu.h - what coral_sketch.cpp (the C ABI of the minimizer sketch) calls in coral_sketch.hip (the device backend).
// Every function returns a CORAL_* code and leaves the reason in `err`.
#ifndef CORAL_SKETCH_GPU_H
#define CORAL_SKETCH_GPU_H

#include <stdint.h>

#include <string>
#include <vector>

#include "coral_sketch_host.h"

namespace coral_sketch_gpu {

struct Device;                       // a device session: its streams, events, pinned staging buffers and the carved workspace

int64_t workspace_bytes(int64_t staging_bytes);
void geometry(int32_t *out);
int open(int k, int w, int device, const uint32_t *bitmap, uint64_t *out_key, uint64_t *out_value, int64_t capacity, int64_t staging_bytes, void *workspace, int64_t workspace_bytes,
         void *stream, Device **out, std::string &err);
int feed(Device *d, const uint8_t *bytes, int64_t n, std::string &err);
// waits for the stream; the minimizers found (written up to the capacity), the contigs and seconds[0..3] = upload, symbols +
// contig table, sketch, the last tile
int finish(Device *d, uint64_t *n_out, std::vector<int64_t> &lengths, coral_sketch::Names &names, double *seconds, std::string &err);
void close(Device *d);

// the index, on device arrays
int64_t sort_workspace_bytes(int64_t n);
int sort(int device, uint64_t *keys, uint64_t *values, int64_t n, int k, void *workspace, int64_t workspace_bytes, void *stream, std::string &err);
int lookup(int device, const uint64_t *sorted, int64_t n, const uint64_t *qkey, int64_t nq, int64_t *first, int64_t *count, void *stream, std::string &err);
int64_t anchors_workspace_bytes(int64_t nq);
int anchors(int device, const uint64_t *sorted, const uint64_t *values, int64_t n, const uint32_t *query, const uint32_t *qpos, const uint8_t *qstrand, const uint64_t *qkey, int64_t nq,
            int64_t max_occ, int64_t capacity, uint64_t *a_query, uint64_t *a_ref, void *workspace, int64_t workspace_bytes, void *stream, int64_t *n_out, std::string &err);

}  // namespace coral_sketch_gpu
#endif /* CORAL_SKETCH_GPU_H */
