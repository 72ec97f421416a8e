// galileo-sdr-sim: the output side of the run loop -- the pinned buffers the batches are copied into and the sink that drains them.
#pragma once
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

struct Slot {  // one pinned host buffer of the double-buffered sink
    int16_t *host = nullptr;
    size_t bytes = 0;
    int n_elem = 1;     // --array: the elements' outputs lie one behind the other, `stride` bytes apart, `bytes` of each are the batch's;
    size_t stride = 0;  // the writer thread splits them into the elements' files
    hipEvent_t copied[2] = {nullptr, nullptr};  // the batch leaves the GPU in two halves on two copy streams
    bool full = false;
};

// ---- the output ------------------------------------------------------------------------------------------------
// Regular file: ftruncate to the final size + one shared mapping; put() has `n_workers` threads copy disjoint pieces.
// Anything else (stdout, pipe, device): sequential write().
class Sink {
public:
    ~Sink()
    {
        close_workers();
        if (prealloc_.joinable()) {
            stop_prealloc_ = true;
            prealloc_.join();
        }
    }

    bool open(const char *path, size_t total_bytes, int n_workers)
    {
        total_ = total_bytes;
        if (strcmp(path, "-") == 0) {
            fd_ = STDOUT_FILENO;
            own_fd_ = false;
        } else {
            fd_ = ::open(path, O_RDWR | O_CREAT | O_TRUNC, 0644);
            if (fd_ < 0) fd_ = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);  // write-only sinks (devices, FIFOs)
            if (fd_ < 0) return false;
            own_fd_ = true;
        }
        struct stat sb;
        const char *force = getenv("GAL_SINK");  // "stream": never map (A/B measurements)
        if (own_fd_ && fstat(fd_, &sb) == 0 && S_ISREG(sb.st_mode) && total_ > 0 && n_workers > 0 &&
            !(force && strcmp(force, "stream") == 0) && ftruncate(fd_, (off_t)total_) == 0) {
            void *m = mmap(nullptr, total_, PROT_READ | PROT_WRITE, MAP_SHARED, fd_, 0);
            if (m != MAP_FAILED) {
                map_ = (char *)m;
                for (int i = 0; i < n_workers; ++i) workers_.emplace_back([this, i] { worker(i); });
            } else if (ftruncate(fd_, 0) != 0) {
                return false;
            }
        }
        // Sequential sink into a regular file of known size: a helper thread allocates the file's pages ahead of the writes
        // (fallocate, size kept: the file grows as it is written), 64 MB at a time, WHILE the device starts up -- the run's
        // write()s then copy into pages that exist (tmpfs on the MI355X host: 1.19 GB allocate 70 ms, write() into allocated
        // pages 130 ms, write() that allocates as it goes 190 ms; profiles/archive/r03j_sink_probe.log).  Failure is not an error:
        // the writes allocate for themselves then.  GAL_SINK=noprealloc turns it off.
        if (!map_ && own_fd_ && fstat(fd_, &sb) == 0 && S_ISREG(sb.st_mode) && total_ > 0 &&
            !(force && (strcmp(force, "noprealloc") == 0))) {
            prealloc_ = std::thread([this] {
                const size_t step = (size_t)64 << 20;
                for (size_t o = 0; o < total_ && !stop_prealloc_.load(std::memory_order_relaxed); o += step) {
                    const size_t n = total_ - o < step ? total_ - o : step;
                    if (fallocate(fd_, FALLOC_FL_KEEP_SIZE, (off_t)o, (off_t)n) != 0) break;
                }
            });
        }
        return true;
    }
    bool mapped() const { return map_ != nullptr; }
    int workers() const { return (int)workers_.size(); }

    // appends `bytes` from `src`; returns false on an I/O error
    bool put(const char *src, size_t bytes)
    {
        if (map_) {
            if (pos_ + bytes > total_) return false;
            {
                std::lock_guard<std::mutex> lk(mu_);
                job_src_ = src;
                job_dst_ = map_ + pos_;
                job_bytes_ = bytes;
                job_next_ = 0;
                job_left_ = (int)workers_.size();
                ++job_id_;
            }
            cv_.notify_all();
            std::unique_lock<std::mutex> lk(mu_);
            done_cv_.wait(lk, [&] { return job_left_ == 0; });
            pos_ += bytes;
            return true;
        }
        while (bytes) {
            const ssize_t n = ::write(fd_, src, bytes < ((size_t)1 << 30) ? bytes : ((size_t)1 << 30));
            if (n < 0) {
                if (errno == EINTR) continue;
                return false;
            }
            src += n;
            bytes -= (size_t)n;
            pos_ += (size_t)n;
        }
        return true;
    }

    // all data are in the file (mapped sink: in its page cache); a run that stopped early is cut to what was written
    bool finish()
    {
        close_workers();
        bool ok = true;
        if (prealloc_.joinable()) {
            stop_prealloc_ = true;
            prealloc_.join();
            // a run that stopped early (SIGINT, error): give back the pages allocated beyond what was written
            if (pos_ < total_ && ftruncate(fd_, (off_t)pos_) != 0) ok = false;
        }
        if (map_) {
            munmap(map_, total_);
            map_ = nullptr;
            if (pos_ < total_ && ftruncate(fd_, (off_t)pos_) != 0) ok = false;
        }
        if (own_fd_ && fd_ >= 0 && ::close(fd_) != 0) ok = false;
        fd_ = -1;
        return ok;
    }

private:
    static constexpr size_t kPiece = (size_t)2 << 20;  // 2 MiB: whole huge pages where the file system has them

    void worker(int)
    {
        unsigned long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return quit_ || job_id_ != seen; });
            if (quit_) return;
            seen = job_id_;
            for (;;) {
                const size_t o = job_next_;
                if (o >= job_bytes_) break;
                const size_t n = job_bytes_ - o < kPiece ? job_bytes_ - o : kPiece;
                job_next_ = o + n;
                lk.unlock();
                memcpy(job_dst_ + o, job_src_ + o, n);
                lk.lock();
            }
            if (--job_left_ == 0) done_cv_.notify_all();
        }
    }
    void close_workers()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
        workers_.clear();
    }

    int fd_ = -1;
    bool own_fd_ = false;
    std::thread prealloc_;
    std::atomic<bool> stop_prealloc_{false};
    char *map_ = nullptr;
    size_t total_ = 0, pos_ = 0;
    std::vector<std::thread> workers_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    bool quit_ = false;
    unsigned long job_id_ = 0;
    const char *job_src_ = nullptr;
    char *job_dst_ = nullptr;
    size_t job_bytes_ = 0, job_next_ = 0;
    int job_left_ = 0;
};
