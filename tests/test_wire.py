"""Wire schema built without protoc: encodings pinned byte-for-byte against
hand-computed protobuf wire format of node_service.proto (reference schema)."""
import numpy as np
import pytest
import torch

from distributed_neural_networks_amd.wire import codec, proto


def _varint(n):
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _ld(field, payload):  # length-delimited field
    return _varint((field << 3) | 2) + _varint(len(payload)) + payload


def test_method_paths():
    assert proto.method_path("SendTensor") == "/node_service.NodeService/SendTensor"
    assert proto.FILE_DESCRIPTOR.package == "node_service"
    names = [m.name for m in proto.FILE_DESCRIPTOR.services_by_name["NodeService"].methods]
    assert names == ["SendMessage", "HealthCheck", "SendTensor"]


def test_tensor_request_bytes():
    data = np.arange(6, dtype=np.float32).reshape(2, 3)
    req = proto.TensorRequest(request_id="cifar_pipe_2node_001", tensor=codec.encode(data))
    t = _ld(1, data.tobytes()) + _ld(2, _varint(2) + _varint(3)) + _ld(3, b"float32")  # packed repeated int32
    expect = _ld(1, b"cifar_pipe_2node_001") + _ld(2, t)
    assert req.SerializeToString() == expect


def test_response_optional_presence():
    r = proto.TensorResponse(status="ok")
    assert not r.HasField("result_tensor")
    r2 = proto.TensorResponse.FromString(proto.TensorResponse(status="x", result_tensor=proto.Tensor()).SerializeToString())
    assert r2.HasField("result_tensor")


def test_misc_messages():
    assert proto.HealthCheckResponse(is_healthy=True).SerializeToString() == b"\x08\x01"
    m = proto.MessageRequest(sender_id="a", message_text="hi")
    assert m.SerializeToString() == _ld(1, b"a") + _ld(2, b"hi")
    assert proto.Empty().SerializeToString() == b""


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.int64, np.int32, np.float16, np.uint8])
def test_codec_numpy_roundtrip(dt):
    a = (np.random.default_rng(0).standard_normal((3, 5)) * 10).astype(dt)
    m = codec.encode(a)
    assert m.dtype == str(np.dtype(dt))
    assert np.array_equal(codec.decode(m).numpy(), a)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2])
def test_codec_torch_only_dtypes(dt):
    t = torch.randn(4, 7).to(dt)
    m = codec.encode(t)
    assert m.dtype in ("bfloat16", "float8_e4m3fn", "float8_e5m2")
    back = codec.decode(m)
    assert back.dtype == dt and torch.equal(back.view(torch.uint8), t.view(torch.uint8))


def test_large_message_roundtrip():
    # the reference dies at 4 MiB (RESOURCE_EXHAUSTED); the codec itself has no cap
    a = np.zeros((300, 4096), dtype=np.float32)
    m = proto.TensorRequest(request_id="big", tensor=codec.encode(a))
    b = proto.TensorRequest.FromString(m.SerializeToString())
    assert codec.decode(b.tensor).shape == (300, 4096)


def _proto_file_tables():
    """Messages and services of the package's ``wire/node_service.proto`` (the
    schema as text; no protoc here), in the form ``test_descriptor_matches_proto_file_field_by_field``
    compares: per field (name, number, type, label, type_name, proto3_optional, oneof_index)."""
    import os
    import re
    from google.protobuf.descriptor_pb2 import FieldDescriptorProto as F
    src = open(os.path.join(os.path.dirname(proto.__file__), "node_service.proto")).read()
    src = re.sub(r"//[^\n]*", "", src)
    scalar = {"string": F.TYPE_STRING, "bool": F.TYPE_BOOL, "bytes": F.TYPE_BYTES, "int32": F.TYPE_INT32}
    package = re.search(r"package\s+([\w.]+)\s*;", src).group(1)
    syntax = re.search(r'syntax\s*=\s*"(\w+)"\s*;', src).group(1)
    msgs = {}
    for name, body in re.findall(r"message\s+(\w+)\s*\{([^}]*)\}", src):
        fields = []
        for mod, typ, fname, num in re.findall(r"(optional|repeated)?\s*([\w.]+)\s+(\w+)\s*=\s*(\d+)\s*;", body):
            fields.append((fname, int(num), scalar.get(typ, F.TYPE_MESSAGE),
                           F.LABEL_REPEATED if mod == "repeated" else F.LABEL_OPTIONAL,
                           "" if typ in scalar else f".{package}.{typ}", mod == "optional",
                           0 if mod == "optional" else None))
        msgs[name] = fields
    svcs = {}
    for name, body in re.findall(r"service\s+(\w+)\s*\{([^}]*)\}", src):
        svcs[name] = [(m, f".{package}.{i}", f".{package}.{o}", False, False) for m, i, o in
                      re.findall(r"rpc\s+(\w+)\s*\(\s*(\w+)\s*\)\s*returns\s*\(\s*(\w+)\s*\)\s*;", body)]
    return package, syntax, msgs, svcs


def test_descriptor_matches_proto_file_field_by_field():
    """The descriptor that ``wire/proto.py`` assembles by hand is the one the
    committed ``node_service.proto`` declares: every message, field number,
    type, label, proto3 ``optional`` and every service method."""
    from google.protobuf import descriptor_pb2
    package, syntax, want_msgs, want_svcs = _proto_file_tables()
    ours = descriptor_pb2.FileDescriptorProto()
    proto.FILE_DESCRIPTOR.CopyToProto(ours)
    assert ours.package == package == "node_service"
    assert ours.syntax == syntax
    assert len(want_msgs) == 7 and sum(len(f) for f in want_msgs.values()) == 11  # the parser saw the whole file

    def msgs(fd):
        return {m.name: [(f.name, f.number, f.type, f.label, f.type_name, f.proto3_optional, f.oneof_index
                          if f.HasField("oneof_index") else None) for f in m.field] for m in fd.message_type}
    assert msgs(ours) == want_msgs

    def svcs(fd):
        return {s.name: [(x.name, x.input_type, x.output_type, x.client_streaming, x.server_streaming)
                         for x in s.method] for s in fd.service}
    assert svcs(ours) == want_svcs and len(want_svcs["NodeService"]) == 3
