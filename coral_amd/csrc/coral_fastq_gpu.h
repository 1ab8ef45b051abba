// coral_fastq_gpu.h - what coral_fastq.cpp (the C ABI of the read QC and the read filter on FASTQ text) calls in coral_fastq.hip (the
// device backend).  Every function returns a CORAL_* code and leaves the reason in `err`.
#ifndef CORAL_FASTQ_GPU_H
#define CORAL_FASTQ_GPU_H

#include <stdint.h>

#include <string>

#include "coral_fastq_host.h"

namespace coral_fastq_gpu {

struct Device;                       // a device session: its copy stream, events, pinned staging buffers and the carved workspace

int64_t workspace_bytes(int64_t staging_bytes);
void geometry(int32_t *out);
int open(int device, const coral_fastq::Thresholds &thr, int fd, int64_t staging_bytes, void *hist, void *workspace, int64_t workspace_bytes, void *stream, Device **out, std::string &err);
int feed(Device *d, const uint8_t *bytes, int64_t n, std::string &err);
// waits for the stream; seconds[0..3] = upload, scan + walk, accumulate, write
int finish(Device *d, double *seconds, std::string &err);
const coral_fastq::Rows &rows(const Device *d);
void close(Device *d);

}  // namespace coral_fastq_gpu
#endif /* CORAL_FASTQ_GPU_H */
