/*
 * Stand-in for <glog/logging.h>, written for this project.
 *
 * TEST INFRASTRUCTURE ONLY.  It exists so that the SwitchML reference's
 * client library (which needs glog only through a handful of macros) can be
 * compiled UNMODIFIED into oracle/_ref/ and used as the bit-level pin of the
 * oracle.  It covers exactly what the reference's dummy-backend
 * client library uses:
 *
 *   LOG(sev), LOG_IF(sev, c), VLOG(n), VLOG_IF(n, c), DVLOG(n), CHECK(c),
 *   VLOG_IS_ON(n), DCHECK_IS_ON(), DECLARE_string(name),
 *   google::InitGoogleLogging, google::LogMessageVoidify.
 *
 * Every message is discarded, except that a FATAL one is printed to stderr
 * and aborts, as glog's does.  Verbose logging is always off, so the operands
 * of VLOG / DVLOG are never evaluated, as with glog when the level is off.
 */
#ifndef SML_STANDIN_GLOG_LOGGING_H_
#define SML_STANDIN_GLOG_LOGGING_H_

/* Real glog drags these in; the reference's utils.h relies on that. */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <ostream>
#include <sstream>
#include <string>
#include <vector>

namespace google {

/* Swallows every operand without formatting it. */
class NullStream {
  public:
    template <typename T>
    NullStream& operator<<(const T&) { return *this; }
    NullStream& operator<<(std::ostream& (*)(std::ostream&)) { return *this; }
};

/* Formats the message; prints it and aborts when the statement ends. */
class FatalStream {
  public:
    FatalStream(const char* file, int line) { ss_ << "F " << file << ":" << line << "] "; }
    [[noreturn]] ~FatalStream() {
        std::fprintf(stderr, "%s\n", ss_.str().c_str());
        std::fflush(stderr);
        std::abort();
    }
    template <typename T>
    FatalStream& operator<<(const T& v) { ss_ << v; return *this; }
    FatalStream& operator<<(std::ostream& (*m)(std::ostream&)) { ss_ << m; return *this; }

  private:
    std::ostringstream ss_;
};

/* Gives both arms of the conditional macros the type void. */
class LogMessageVoidify {
  public:
    void operator&(const NullStream&) {}
    void operator&(const FatalStream&) {}
};

inline void InitGoogleLogging(const char*) {}

}  // namespace google

#define SML_GLOG_STREAM_INFO google::NullStream()
#define SML_GLOG_STREAM_WARNING google::NullStream()
#define SML_GLOG_STREAM_ERROR google::NullStream()
#define SML_GLOG_STREAM_FATAL google::FatalStream(__FILE__, __LINE__)

#define LOG(severity) SML_GLOG_STREAM_##severity
#define LOG_IF(severity, condition) \
    !(condition) ? (void)0 : google::LogMessageVoidify() & LOG(severity)
#define CHECK(condition) LOG_IF(FATAL, !(condition)) << "Check failed: " #condition " "

#define VLOG_IS_ON(verboselevel) false
#define VLOG(verboselevel) true ? (void)0 : google::LogMessageVoidify() & LOG(INFO)
#define VLOG_IF(verboselevel, condition) VLOG(verboselevel)
#define DVLOG(verboselevel) VLOG(verboselevel)

#ifdef NDEBUG
#define DCHECK_IS_ON() 0
#else
#define DCHECK_IS_ON() 1
#endif

#define DECLARE_string(name) extern std::string FLAGS_##name

#endif  /* SML_STANDIN_GLOG_LOGGING_H_ */
