// coral_comp_gpu.h - what coral_comp.cpp (the C ABI of the reference's per-bin composition) calls in coral_comp.hip (the device
// backend).  Every function returns a CORAL_* code and leaves the reason in `err`.
#ifndef CORAL_COMP_GPU_H
#define CORAL_COMP_GPU_H

#include <stdint.h>

#include <string>
#include <vector>

#include "coral_comp_host.h"

namespace coral_comp_gpu {

struct Device;                       // a device session: its streams, events, pinned staging buffers and the carved workspace

int64_t workspace_bytes(int64_t staging_bytes);
void geometry(int32_t *out);
int open(int64_t bin_size, int device, uint32_t *gc, uint32_t *at, uint32_t *masked, int64_t capacity, int64_t staging_bytes, void *workspace, int64_t workspace_bytes,
         void *stream, Device **out, std::string &err);
int feed(Device *d, const uint8_t *bytes, int64_t n, std::string &err);
// waits for the stream; the statistics, the contigs and seconds[0..3] = upload, ordinals + contigs, count, 0
int finish(Device *d, coral_comp::Stats &st, std::vector<int64_t> &lengths, coral_comp::Names &names, double *seconds, std::string &err);
void close(Device *d);

}  // namespace coral_comp_gpu
#endif /* CORAL_COMP_GPU_H */
