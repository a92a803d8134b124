// amhip_file_io.cc -- whole files to and from host memory, for every writer and reader of the library
// (declared in amhip_common.h).  Host only.  The status enum has no I/O code: a file that cannot be
// written or read is AMHIP_ERR_ARG with the caller's name, the file's name and errno's text.
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "aerial_mapper_hip.h"

namespace amhip {

// (as amhip_common.h declares them; that header needs HIP, this source is compiled without)
void set_last_error(const std::string& msg);
int write_file(const char* what, const char* filename, const uint8_t* data, size_t size);
int read_file(const char* what, const char* filename, std::vector<uint8_t>* out);

static int io_failure(const char* what, const std::string& text) {
  set_last_error(std::string(what) + ": " + text);
  return AMHIP_ERR_ARG;
}

static int write_failure(const char* what, const char* filename, int err) {
  return io_failure(what, std::string("cannot write ") + filename + ": " + std::strerror(err));
}

int write_file(const char* what, const char* filename, const uint8_t* data, size_t size) {
  const int fd = ::open(filename, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) return write_failure(what, filename, errno);
  size_t done = 0;
  while (done < size) {
    const ssize_t w = ::write(fd, data + done, size - done);
    if (w < 0 && errno == EINTR) continue;
    if (w < 0) {
      const int err = errno;   // (close() below may change it)
      (void)::close(fd);
      return write_failure(what, filename, err);
    }
    done += (size_t)w;
  }
  if (::close(fd) != 0) return write_failure(what, filename, errno);
  return AMHIP_OK;
}

int read_file(const char* what, const char* filename, std::vector<uint8_t>* out) {
  FILE* f = std::fopen(filename, "rb");
  if (!f) return io_failure(what, std::string("cannot open ") + filename + ": " + std::strerror(errno));
  out->clear();
  uint8_t block[1 << 16];
  size_t got;
  while ((got = std::fread(block, 1, sizeof(block), f)) > 0) out->insert(out->end(), block, block + got);
  const bool failed = std::ferror(f) != 0;
  std::fclose(f);
  if (failed) return io_failure(what, std::string("cannot read ") + filename);
  return AMHIP_OK;
}

}  // namespace amhip
