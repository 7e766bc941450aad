// syntax-check stand-in for xmlrpcpp's XmlRpcValue (the part a node needs to read list / struct parameters)
#ifndef XMLRPCVALUE_STUB_H
#define XMLRPCVALUE_STUB_H
#include <string>
namespace XmlRpc {
class XmlRpcValue {
   public:
    enum Type { TypeInvalid, TypeBoolean, TypeInt, TypeDouble, TypeString, TypeDateTime, TypeBase64, TypeArray, TypeStruct };
    XmlRpcValue();
    Type const &getType() const;
    int size() const;
    bool hasMember(const std::string &name) const;
    XmlRpcValue &operator[](int i);
    XmlRpcValue &operator[](const std::string &k);
    XmlRpcValue &operator[](const char *k);
    operator bool &();
    operator int &();
    operator double &();
    operator std::string &();
};
}  // namespace XmlRpc
#endif
