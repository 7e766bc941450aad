// syntax-check stand-in for xmlrpcpp's XmlRpcException
#ifndef XMLRPCEXCEPTION_STUB_H
#define XMLRPCEXCEPTION_STUB_H
#include <string>
namespace XmlRpc {
class XmlRpcException {
   public:
    XmlRpcException(const std::string &message, int code = -1);
    const std::string &getMessage() const;
    int getCode() const;
};
}  // namespace XmlRpc
#endif
